"""ctypes binding of libsbm_hip.so (the C ABI declared in include/sbm.h).

There is no CPU fallback: if the shared library is missing, or no MI355X is
visible, every call raises.  The library is built in-tree by
``__graft_entry__.build()`` / ``make -C shape_based_matching_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .templates import FEATURE_DTYPE, LEVEL_DTYPE, MATCH_DTYPE, TemplateSet

TRAIN_FEATURE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("label", "<i4"), ("theta", "<f4")])  # sbm_train_feature

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsbm_hip.so")
SBM_MAX_LEVELS = 8

# every symbol include/sbm.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "sbm_last_error", "sbm_abi_version", "sbm_create", "sbm_destroy", "sbm_upload_templates",
    "sbm_select_classes", "sbm_select_range", "sbm_match", "sbm_match_device", "sbm_match_batch_device", "sbm_canonicalize",
    "sbm_build_pyramid", "sbm_set_quantized", "sbm_get_quantized", "sbm_get_linear_memories",
    "sbm_level_dims", "sbm_match_templates", "sbm_quantized_orientations", "sbm_pyrdown", "sbm_spread",
    "sbm_compute_response_maps", "sbm_linearize", "sbm_similarity", "sbm_similarity_local",
    "sbm_set_profiling", "sbm_get_timings", "sbm_coarse_bytes", "sbm_get_stats",
    "sbm_set_result_mirror", "sbm_set_graph_mode", "sbm_set_quantize_mode", "sbm_resize_linear",
    "sbm_match_templates_device", "sbm_orientation_bins",
    "sbm_comm_unique_id", "sbm_comm_init", "sbm_comm_destroy", "sbm_match_device_sharded", "sbm_match_batch_device_sharded",
    "sbm_match_batch_device_banded", "sbm_pin_host_buffer", "sbm_unpin_host_buffer",
    "sbm_select_templates", "sbm_partition_templates", "sbm_match_sharded",
    "sbm_match_batch_host", "sbm_match_batch_host_begin", "sbm_match_batch_host_end", "sbm_extract_local_maxima",
    "sbm_train_batch", "sbm_train_batch_device",
    "sbm_train_ragged", "sbm_train_ragged_device", "sbm_train_sweep", "sbm_train_sweep_device",
    "sbm_train_rotate", "sbm_train_rotate_device",
    "sbm_set_pipeline_depth", "sbm_set_coarse_mode", "sbm_set_refine_order", "sbm_set_refine_bits", "sbm_get_coarse_bitplanes",
    "sbm_comm_count", "sbm_match_templates_device_sharded", "sbm_graph_count",
    "sbm_nms_batch_device", "sbm_match_batch_host_end_nms",
    "sbm_match_batch_device_masked", "sbm_match_batch_host_begin_masked", "sbm_match_batch_host_masked", "sbm_get_quantized_frame",
    "sbm_get_coarse_form",
    "sbm_get_source_form",
    "sbm_get_source_retention",
    "sbm_get_refine_form",
    "sbm_get_sparse_items",
    "sbm_get_sparse_list", "sbm_set_sparse_list_rows",
    "sbm_match_batch_device_ptrs",
    "sbm_match_batch_device_planes",
    "sbm_get_level_build",
    "sbm_get_level_stored",
    "sbm_upload_templates_device", "sbm_get_templates", "sbm_get_template_table",
    "sbm_upload_verify_patches", "sbm_get_verify_patch", "sbm_verify_batch_device", "sbm_verify_batch_device_ptrs",
    "sbm_verify_batch_device_planes", "sbm_match_batch_host_verified",
]

# sbm_match_batch_device_ptrs flags: the caller promises that every frame pointer is a multiple of 4
SBM_PTRS_ALIGNED4 = 1


class SbmConfig(C.Structure):
    _fields_ = [
        ("n_levels", C.c_int32),
        ("T", C.c_int32 * SBM_MAX_LEVELS),
        ("weak_threshold", C.c_float),
        ("device_id", C.c_int32),
        ("max_candidates", C.c_int64),
    ]


class SbmNmsParams(C.Structure):
    """sbm_nms_params: cv_dnn::NMSBoxes' arguments (include/nms.hpp)"""
    _fields_ = [
        ("score_threshold", C.c_float),
        ("nms_threshold", C.c_float),
        ("eta", C.c_float),
        ("top_k", C.c_int32),
    ]


class SbmVerifyPatch(C.Structure):
    """sbm_verify_patch: the gray fiducial patch of one template label (32 bytes)"""
    _fields_ = [
        ("class_idx", C.c_int32),
        ("template_id", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("stride", C.c_int32),
        ("reserved", C.c_int32),
        ("gray", C.c_void_p),
    ]


class SbmVerifyParams(C.Structure):
    """sbm_verify_params: the verify stage's threshold (the reference: 0.8) and what becomes of unverifiable records"""
    _fields_ = [
        ("min_corr", C.c_double),
        ("keep_unverified", C.c_int32),
        ("reserved", C.c_int32),
    ]


class SbmTrainImage(C.Structure):
    """sbm_train_image: one image of a ragged training call (48 bytes)"""
    _fields_ = [
        ("img", C.c_void_p),
        ("mask", C.c_void_p),
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("stride", C.c_int32),
        ("num_features", C.c_int32),
        ("feat_first", C.c_int64),
        ("feat_cap", C.c_int64),
    ]


class SbmTrainScale(C.Structure):
    """sbm_train_scale: one scale of a training sweep (40 bytes)"""
    _fields_ = [
        ("fx", C.c_double),
        ("fy", C.c_double),
        ("num_features", C.c_int32),
        ("reserved", C.c_int32),
        ("feat_first", C.c_int64),
        ("feat_cap", C.c_int64),
    ]


class SbmRotateBase(C.Structure):
    """sbm_rotate_base: one trained pyramid of a rotate call and where its rotations go (48 bytes)"""
    _fields_ = [
        ("levels", C.c_void_p),
        ("feats", C.c_void_p),
        ("status", C.c_void_p),
        ("center_x", C.c_float),
        ("center_y", C.c_float),
        ("out_first", C.c_int64),
        ("out_cap", C.c_int64),
    ]


class SbmTemplateSource(C.Structure):
    """sbm_template_source: a run of trained pyramids of one class in device memory (56 bytes)"""
    _fields_ = [
        ("d_levels", C.c_void_p),
        ("d_feats", C.c_void_p),
        ("d_status", C.c_void_p),
        ("n_pyramids", C.c_int32),
        ("class_idx", C.c_int32),
        ("feat_first", C.c_int64),
        ("feat_pitch", C.c_int64),
        ("feat_cap", C.c_int64),
    ]


# sbm_get_template_table's tables, in its order, with the element type of each
TEMPLATE_TABLES = (("tls", np.int32), ("fxy", np.uint32), ("flabel", np.uint8), ("flevel", np.uint8), ("fxy_s", np.uint32), ("flabel_s", np.uint8),
                   ("fcls", np.uint16), ("fext", np.uint32), ("class", np.int32), ("tid", np.int32))


class SbmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libsbm_hip error {code}: {msg}")
        self.code = code


_lib = None


def _one_hip_runtime_per_process() -> str:
    """PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7) and link it
    by the unversioned file name, so it is never matched to a system runtime that is already loaded: a process that loads
    libsbm_hip.so (NEEDED libamdhip64.so.7 -> /opt/rocm) FIRST and imports torch LATER ends up with two HIP runtimes, and
    the second one to initialise finds no device ("No HIP GPUs are available" from torch.cuda, round 2).  The other order
    is fine: with torch's copy loaded first the loader resolves libsbm_hip's NEEDED entry to it by SONAME.  So, when a
    torch with a bundled runtime is installed, make that order the only one: map torch's copy before libsbm_hip.so --
    whether or not torch has been imported yet (it need not be, and is not imported here).  SBM_HIP_RUNTIME=system
    keeps the system runtime (processes that never import torch)."""
    if os.environ.get("SBM_HIP_RUNTIME", "") == "system":
        return "system"
    import importlib.util
    import sys

    t = sys.modules.get("torch")
    if t is not None:
        base = os.path.dirname(t.__file__)
    else:
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        if spec is None or not spec.submodule_search_locations:
            return "system"
        base = list(spec.submodule_search_locations)[0]
    rt = os.path.join(base, "lib", "libamdhip64.so")
    if not os.path.exists(rt):
        return "system"
    # Only a runtime of the SONAME libsbm_hip.so was linked against may stand in for it: another SONAME would still give
    # two runtimes, and mapping it would be pointless.  Both names are read from the ELF dynamic sections.
    want = [n for n in _elf_dynamic_strings(LIB_PATH, 1) if n.startswith("libamdhip64")]   # DT_NEEDED
    have = _elf_dynamic_strings(rt, 14)                                                      # DT_SONAME
    if want and have and have[0] not in want:
        import warnings

        warnings.warn(f"torch bundles {have[0]} but libsbm_hip.so needs {want[0]}: keeping the system HIP runtime "
                      "(import torch before creating a context, or expect two runtimes in this process)")
        return "system"
    C.CDLL(rt, mode=C.RTLD_GLOBAL)
    return rt


def _elf_dynamic_strings(path: str, tag: int):
    """the strings of the ELF64 little-endian dynamic entries with this tag (1 = DT_NEEDED, 14 = DT_SONAME); [] on any surprise"""
    import struct

    try:
        with open(path, "rb") as f:
            data = f.read()
        if data[:6] != b"\x7fELF\x02\x01":
            return []
        shoff, = struct.unpack_from("<Q", data, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
        secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
        out = []
        for sec in secs:
            if sec[1] != 6:  # SHT_DYNAMIC
                continue
            strtab = secs[sec[6]]  # sh_link
            for off in range(sec[4], sec[4] + sec[5], 16):
                t, v = struct.unpack_from("<qQ", data, off)
                if t == 0:
                    break
                if t == tag:
                    s0 = strtab[4] + v
                    out.append(data[s0:data.index(b"\0", s0)].decode())
        return out
    except Exception:
        return []


HIP_RUNTIME = None  # which HIP runtime lib() made the process's one: "system" or the path of torch's copy


def lib() -> C.CDLL:
    """Load libsbm_hip.so; raises if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension is not built (run __graft_entry__.build()); "
            "shape_based_matching_amd has no CPU fallback"
        )
    global HIP_RUNTIME
    HIP_RUNTIME = _one_hip_runtime_per_process()
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.sbm_last_error.restype = C.c_char_p
    L.sbm_abi_version.restype = i32
    L.sbm_create.argtypes = [C.POINTER(SbmConfig), C.POINTER(vp)]
    L.sbm_destroy.argtypes = [vp]
    L.sbm_destroy.restype = None
    L.sbm_upload_templates.argtypes = [vp, i32, vp, vp, i64, vp, vp]
    L.sbm_select_classes.argtypes = [vp, vp, i32]
    L.sbm_select_range.argtypes = [vp, i32, i32]
    L.sbm_match.argtypes = [vp, vp, i32, i32, i32, i32, vp, f32, vp, i64, C.POINTER(i64)]
    L.sbm_match_device.argtypes = [vp, vp, i32, i32, i32, i32, vp, f32, vp, i64, vp, vp]
    L.sbm_match_batch_device.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, f32, vp, i64, vp, vp]
    L.sbm_match_batch_device_masked.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, i64, f32, vp, i64, vp, vp]
    L.sbm_match_batch_device_ptrs.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, f32, vp, i64, vp, vp]
    L.sbm_match_batch_device_planes.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, f32, vp, i64, vp, vp]
    L.sbm_match_batch_host_begin_masked.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, f32, i64, i32]
    L.sbm_match_batch_host_masked.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, f32, vp, i64, vp, i32]
    L.sbm_get_quantized_frame.argtypes = [vp, i32, i32, vp]
    L.sbm_canonicalize.argtypes = [vp, i64]
    L.sbm_canonicalize.restype = i64
    L.sbm_build_pyramid.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.sbm_set_quantized.argtypes = [vp, i32, vp, i32, i32]
    L.sbm_get_quantized.argtypes = [vp, i32, vp]
    L.sbm_get_linear_memories.argtypes = [vp, i32, vp, i64, C.POINTER(i64)]
    L.sbm_get_coarse_bitplanes.argtypes = [vp, i32, vp, i64]
    L.sbm_get_coarse_form.argtypes = [vp, vp]
    L.sbm_get_source_form.argtypes = [vp, vp]
    L.sbm_get_source_retention.argtypes = [vp, vp]
    L.sbm_get_sparse_items.argtypes = [vp, vp]
    L.sbm_get_sparse_list.argtypes = [vp, vp]
    L.sbm_get_refine_form.argtypes = [vp, i32, vp]
    L.sbm_get_level_build.argtypes = [vp, i32, vp]
    L.sbm_get_level_stored.argtypes = [vp, i32, i32, i32, vp, i64, C.POINTER(i64)]
    L.sbm_level_dims.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.sbm_match_templates.argtypes = [vp, f32, vp, i64, C.POINTER(i64)]
    L.sbm_quantized_orientations.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp, vp, vp]
    L.sbm_pyrdown.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.sbm_orientation_bins.argtypes = [vp, vp, vp, i64, vp]
    L.sbm_spread.argtypes = [vp, vp, i32, i32, i32, vp]
    L.sbm_compute_response_maps.argtypes = [vp, vp, i32, i32, vp]
    L.sbm_linearize.argtypes = [vp, vp, i32, i32, i32, vp]
    L.sbm_similarity.argtypes = [vp, i32, vp]
    L.sbm_similarity_local.argtypes = [vp, i32, i32, i32, i32, vp]
    L.sbm_set_profiling.argtypes = [vp, i32]
    L.sbm_get_timings.argtypes = [vp, vp, vp, i32, C.POINTER(i32)]
    L.sbm_coarse_bytes.argtypes = [vp, C.POINTER(i64)]
    L.sbm_get_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.sbm_set_result_mirror.argtypes = [vp, vp, vp]
    L.sbm_set_graph_mode.argtypes = [vp, i32]
    L.sbm_graph_count.argtypes = [vp, C.POINTER(i32)]
    L.sbm_set_quantize_mode.argtypes = [vp, i32, i32]
    L.sbm_resize_linear.argtypes = [vp, vp, i32, i32, i32, i32, C.c_double, C.c_double, vp, i64, C.POINTER(i32), C.POINTER(i32)]
    L.sbm_match_templates_device.argtypes = [vp, f32, vp, i64, vp, vp]
    L.sbm_comm_unique_id.argtypes = [vp]
    L.sbm_comm_init.argtypes = [vp, i32, i32, vp]
    L.sbm_comm_count.argtypes = [vp, C.POINTER(i32)]
    L.sbm_match_templates_device_sharded.argtypes = [vp, f32, vp, i64, vp, vp, vp]
    L.sbm_comm_destroy.argtypes = [vp]
    L.sbm_match_device_sharded.argtypes = [vp, vp, i32, i32, i32, i32, vp, f32, vp, i64, vp, vp, vp]
    L.sbm_match_batch_device_sharded.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, f32, vp, i64, vp, vp, vp]
    L.sbm_extract_local_maxima.argtypes = [vp, vp, vp, i32, i32, f32, vp, i64, C.POINTER(i64)]
    L.sbm_train_batch_device.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, i64, f32, i32, vp, vp, i64, vp, vp]
    L.sbm_train_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, f32, i32, vp, vp, i64, vp]
    L.sbm_train_ragged_device.argtypes = [vp, vp, i32, i32, f32, vp, vp, vp, vp]
    L.sbm_train_ragged.argtypes = [vp, vp, i32, i32, f32, vp, vp, vp]
    L.sbm_train_sweep_device.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, f32, vp, vp, vp, vp]
    L.sbm_train_sweep.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, f32, vp, vp, vp]
    L.sbm_train_rotate_device.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp]
    L.sbm_train_rotate.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp]
    L.sbm_set_pipeline_depth.argtypes = [vp, i32]
    L.sbm_set_sparse_list_rows.argtypes = [vp, i32]
    L.sbm_set_coarse_mode.argtypes = [vp, i32]
    L.sbm_set_refine_order.argtypes = [vp, i32]
    L.sbm_set_refine_bits.argtypes = [vp, i32]
    L.sbm_select_templates.argtypes = [vp, vp, i32]
    L.sbm_partition_templates.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp]
    L.sbm_match_sharded.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, f32, vp, i64, C.POINTER(i64)]
    L.sbm_match_batch_host_begin.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, f32, i64, i32]
    L.sbm_match_batch_host_end.argtypes = [vp, vp, vp]
    L.sbm_match_batch_host.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, f32, vp, i64, vp, i32]
    L.sbm_pin_host_buffer.argtypes = [vp, vp, i64]
    L.sbm_unpin_host_buffer.argtypes = [vp, vp]
    L.sbm_match_batch_device_banded.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, f32, vp, i64, vp, vp, i32, vp]
    L.sbm_nms_batch_device.argtypes = [vp, vp, vp, i64, i32, i32, i64, C.POINTER(SbmNmsParams), vp, i64, vp, vp]
    L.sbm_match_batch_host_end_nms.argtypes = [vp, C.POINTER(SbmNmsParams), vp, i64, vp]
    L.sbm_upload_templates_device.argtypes = [vp, vp, i32, vp, vp]
    L.sbm_get_templates.argtypes = [vp, vp, vp, i64, vp, vp, C.POINTER(i32), C.POINTER(i64)]
    L.sbm_get_template_table.argtypes = [vp, i32, vp, i64, C.POINTER(i64)]
    pv = C.POINTER(SbmVerifyParams)
    L.sbm_upload_verify_patches.argtypes = [vp, vp, i32]
    L.sbm_get_verify_patch.argtypes = [vp, i32, i32, vp, i64, C.POINTER(C.c_uint64)]
    L.sbm_verify_batch_device.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, i64, pv, vp, vp, i64, vp, vp]
    L.sbm_verify_batch_device_ptrs.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i64, pv, vp, vp, i64, vp, vp]
    L.sbm_verify_batch_device_planes.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i64, pv, vp, vp, i64, vp, vp]
    L.sbm_match_batch_host_verified.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, i64, C.POINTER(SbmNmsParams), pv, vp, vp, i64, vp]
    for name in ABI_SYMBOLS:
        f = getattr(L, name)
        if name not in ("sbm_last_error", "sbm_destroy", "sbm_canonicalize"):
            f.restype = i32
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise SbmError(rc, lib().sbm_last_error().decode("utf-8", "replace"))


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _img(img: np.ndarray) -> Tuple[np.ndarray, int, int, int]:
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        return img, img.shape[0], img.shape[1], 1
    if img.ndim == 3 and img.shape[2] in (1, 3):
        return img, img.shape[0], img.shape[1], img.shape[2]
    raise ValueError("image must be HxW or HxWx{1,3} uint8")


def canonicalize(recs: np.ndarray) -> np.ndarray:
    recs = np.ascontiguousarray(recs, MATCH_DTYPE).copy()
    n = lib().sbm_canonicalize(_p(recs), len(recs))
    return recs[:n]


class Context:
    """One GPU context (``sbm_ctx``)."""

    def __init__(self, T: Sequence[int] = (4, 8), weak_threshold: float = 30.0, device_id: int = 0,
                 max_candidates: int = 0):
        cfg = SbmConfig()
        cfg.n_levels = len(T)
        for i, t in enumerate(T):
            cfg.T[i] = int(t)
        cfg.weak_threshold = float(weak_threshold)
        cfg.device_id = int(device_id)
        cfg.max_candidates = int(max_candidates)
        self.T = [int(t) for t in T]
        self.n_levels = len(T)
        self._h = C.c_void_p()
        _check(lib().sbm_create(C.byref(cfg), C.byref(self._h)))
        self._cap = max_candidates if max_candidates > 0 else 1 << 20
        self.n_templates = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().sbm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- templates ------------------------------------------------------------
    def upload_templates(self, ts: TemplateSet):
        if ts.n_levels != self.n_levels:
            raise ValueError(f"template pyramids have {ts.n_levels} levels, detector has {self.n_levels}")
        levels = np.ascontiguousarray(ts.levels, LEVEL_DTYPE)
        feats = np.ascontiguousarray(ts.features, FEATURE_DTYPE)
        ci = np.ascontiguousarray(ts.class_idx, np.int32)
        ti = np.ascontiguousarray(ts.template_id, np.int32)
        _check(lib().sbm_upload_templates(self._h, ts.n_templates, _p(levels), _p(feats), len(feats), _p(ci), _p(ti)))
        self.n_templates = ts.n_templates

    def upload_templates_device(self, sources: Sequence["SbmTemplateSource"], stream: int = 0) -> np.ndarray:
        """sbm_upload_templates_device: the pyramids of `sources` (records of device addresses, read during the call only), as the
        sbm_train_*_device calls enqueued before on `stream` leave them, become the template set; a pyramid whose status pair
        does not begin with 0 is skipped.  Returns the template index of every input pyramid, -1 for a skipped one."""
        arr = (SbmTemplateSource * max(len(sources), 1))(*sources)
        n = sum(max(int(s.n_pyramids), 0) for s in sources)
        index = np.full(max(n, 1), -1, np.int32)
        _check(lib().sbm_upload_templates_device(self._h, arr, len(sources), _p(index), C.c_void_p(stream) if stream else None))
        index = index[:n]
        self.n_templates = int((index >= 0).sum())
        return index

    def get_templates(self) -> TemplateSet:
        """the installed set in the input form of upload_templates, after either upload (sbm_get_templates)"""
        nt, nf = C.c_int32(0), C.c_int64(0)
        _check(lib().sbm_get_templates(self._h, None, None, 0, None, None, C.byref(nt), C.byref(nf)))
        levels = np.zeros((nt.value, self.n_levels), LEVEL_DTYPE)
        feats = np.zeros(nf.value, FEATURE_DTYPE)
        ci, ti = np.zeros(nt.value, np.int32), np.zeros(nt.value, np.int32)
        _check(lib().sbm_get_templates(self._h, _p(levels), _p(feats), len(feats), _p(ci), _p(ti), C.byref(nt), C.byref(nf)))
        return TemplateSet(self.n_levels, levels, feats, ci, ti)

    def get_template_table(self, which) -> np.ndarray:
        """one of the ten template tables exactly as it lies in device memory (sbm_get_template_table): `which` is its number
        or its name in TEMPLATE_TABLES"""
        if isinstance(which, str):
            which = [name for name, _ in TEMPLATE_TABLES].index(which)
        n = C.c_int64(0)
        _check(lib().sbm_get_template_table(self._h, which, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        _check(lib().sbm_get_template_table(self._h, which, _p(out), out.nbytes, C.byref(n)))
        return out.view(TEMPLATE_TABLES[which][1])

    def select_classes(self, class_idx: Sequence[int]):
        a = np.asarray(list(class_idx), np.int32)
        _check(lib().sbm_select_classes(self._h, _p(a) if len(a) else None, len(a)))

    def select_range(self, first: int, count: int):
        _check(lib().sbm_select_range(self._h, first, count))

    # -- whole path -------------------------------------------------------------
    def match(self, img: np.ndarray, threshold: float, mask: Optional[np.ndarray] = None) -> np.ndarray:
        img, r, c, ch = _img(img)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.empty(self._cap, MATCH_DTYPE)
        n = C.c_int64(0)
        _check(lib().sbm_match(self._h, _p(img), r, c, c * ch, ch, _p(m), C.c_float(threshold), _p(out), self._cap, C.byref(n)))
        return out[: n.value].copy()

    def match_device(self, d_img: int, rows: int, cols: int, stride: int, channels: int, threshold: float,
                     d_out: int, cap: int, d_count: int, stream: int = 0, d_mask: int = 0):
        _check(lib().sbm_match_device(self._h, C.c_void_p(d_img), rows, cols, stride, channels,
                                      C.c_void_p(d_mask) if d_mask else None, C.c_float(threshold),
                                      C.c_void_p(d_out), cap, C.c_void_p(d_count),
                                      C.c_void_p(stream) if stream else None))

    def match_batch_device(self, d_imgs: int, frame_stride: int, n_frames: int, rows: int, cols: int, stride: int,
                           channels: int, threshold: float, d_out: int, cap: int, d_counts: int, stream: int = 0,
                           d_mask: int = 0):
        """n_frames frames (frame f at d_imgs + f*frame_stride) in one launch of every kernel; frame f's records
        at d_out + f*cap records, its {n, overflow} at d_counts + 2*f int32."""
        _check(lib().sbm_match_batch_device(self._h, C.c_void_p(d_imgs), frame_stride, n_frames, rows, cols, stride,
                                            channels, C.c_void_p(d_mask) if d_mask else None, C.c_float(threshold),
                                            C.c_void_p(d_out), cap, C.c_void_p(d_counts),
                                            C.c_void_p(stream) if stream else None))

    def match_batch_device_masked(self, d_imgs: int, frame_stride: int, n_frames: int, rows: int, cols: int, stride: int,
                                  channels: int, d_masks: int, mask_stride: int, threshold: float, d_out: int, cap: int,
                                  d_counts: int, stream: int = 0):
        """match_batch_device with one mask per frame: frame f's mask at d_masks + f*mask_stride bytes (mask_stride 0: one
        mask shared by the frames)"""
        _check(lib().sbm_match_batch_device_masked(self._h, C.c_void_p(d_imgs), frame_stride, n_frames, rows, cols, stride,
                                                   channels, C.c_void_p(d_masks) if d_masks else None, mask_stride,
                                                   C.c_float(threshold), C.c_void_p(d_out), cap, C.c_void_p(d_counts),
                                                   C.c_void_p(stream) if stream else None))

    def match_batch_device_ptrs(self, d_frame_ptrs: int, n_frames: int, rows: int, cols: int, stride: int, channels: int,
                                threshold: float, d_out: int, cap: int, d_counts: int, d_mask_ptrs: int = 0, flags: int = 0,
                                stream: int = 0):
        """match_batch_device for frames that are not one block: d_frame_ptrs is a DEVICE array of n_frames 64-bit addresses
        (entry f: frame f's first pixel), d_mask_ptrs 0 or a device array of n_frames mask addresses (no zero entry); the
        kernels read both on the stream, the host never does.  flags: 0 or SBM_PTRS_ALIGNED4."""
        _check(lib().sbm_match_batch_device_ptrs(self._h, C.c_void_p(d_frame_ptrs) if d_frame_ptrs else None, n_frames, rows, cols,
                                                 stride, channels, C.c_void_p(d_mask_ptrs) if d_mask_ptrs else None, flags,
                                                 C.c_float(threshold), C.c_void_p(d_out), cap, C.c_void_p(d_counts),
                                                 C.c_void_p(stream) if stream else None))

    def match_batch_device_planes(self, d_plane_ptrs: int, n_frames: int, rows: int, cols: int, stride: int, threshold: float,
                                  d_out: int, cap: int, d_counts: int, d_mask_ptrs: int = 0, flags: int = 0, stream: int = 0):
        """match_batch_device_ptrs for planar frames of three channels: d_plane_ptrs is a DEVICE array of 3 * n_frames 64-bit
        addresses (entry 3 f + c: channel c of frame f, in the reference's order B, G, R -- the caller's to choose), stride the bytes
        per row of a plane, d_mask_ptrs as for match_batch_device_ptrs; flags is reserved (0).  torch_frames.plane_table writes
        the table for [B, 3, H, W] tensors."""
        _check(lib().sbm_match_batch_device_planes(self._h, C.c_void_p(d_plane_ptrs) if d_plane_ptrs else None, n_frames, rows, cols,
                                                   stride, C.c_void_p(d_mask_ptrs) if d_mask_ptrs else None, flags,
                                                   C.c_float(threshold), C.c_void_p(d_out), cap, C.c_void_p(d_counts),
                                                   C.c_void_p(stream) if stream else None))

    def nms_batch_device(self, d_recs: int, d_counts: int, cap: int, n_frames: int, d_out: int, out_cap: int, d_out_counts: int,
                         score_threshold: float, nms_threshold: float, eta: float = 1.0, top_k: int = 0, n_parts: int = 1,
                         part_stride: int = 0, stream: int = 0):
        """match epilogue + NMSBoxes per frame on the device (sbm_nms_batch_device): part p, frame f's records at
        d_recs + p*part_stride + f*cap*24 bytes, its {n, overflow} at d_counts + p*part_stride + 8*f; frame f's kept
        records at d_out + f*out_cap records, {n_kept, flags} at d_out_counts + 2*f int32."""
        prm = SbmNmsParams(score_threshold, nms_threshold, eta, top_k)
        _check(lib().sbm_nms_batch_device(self._h, C.c_void_p(d_recs), C.c_void_p(d_counts), cap, n_frames, n_parts, part_stride,
                                          C.byref(prm), C.c_void_p(d_out) if d_out else None, out_cap, C.c_void_p(d_out_counts),
                                          C.c_void_p(stream) if stream else None))

    def match_batch_host_nms(self, frames: Sequence[np.ndarray], threshold: float, score_threshold: float, nms_threshold: float,
                             eta: float = 1.0, top_k: int = 0, cap: int = 1024, out_cap: int = 256, sub_batch: int = 0,
                             mask: Optional[np.ndarray] = None):
        """sbm_match_batch_host_begin + sbm_match_batch_host_end_nms: per frame the NMS-kept records (a list of record
        arrays) and the {n_kept, flags} pairs"""
        arrs = [_img(f) for f in frames]
        r, c, ch = arrs[0][1:]
        assert all(a[1:] == (r, c, ch) for a in arrs)
        ptrs = (C.c_void_p * len(arrs))(*[a[0].ctypes.data for a in arrs])
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.zeros((len(arrs), out_cap), MATCH_DTYPE)
        counts = np.zeros((len(arrs), 2), np.int32)
        prm = SbmNmsParams(score_threshold, nms_threshold, eta, top_k)
        _check(lib().sbm_match_batch_host_begin(self._h, ptrs, len(arrs), r, c, c * ch, ch, _p(m), C.c_float(threshold), cap, sub_batch))
        _check(lib().sbm_match_batch_host_end_nms(self._h, C.byref(prm), _p(out), out_cap, _p(counts)))
        return [out[f, : counts[f, 0]].copy() for f in range(len(arrs))], counts

    def upload_verify_patches(self, patches: Sequence[Tuple[int, int, np.ndarray]]):
        """sbm_upload_verify_patches: (class_idx, template_id, gray patch HxW uint8) per label, each of its template's level-0
        size; an array that is not contiguous along its rows is copied, a row stride is passed as it is.  [] clears the set."""
        arrs = []
        for _, _, g in patches:
            g = np.asarray(g, np.uint8)
            assert g.ndim == 2
            arrs.append(g if g.size == 0 or g.strides[1] == 1 and g.strides[0] >= g.shape[1] else np.ascontiguousarray(g))
        recs = (SbmVerifyPatch * max(len(arrs), 1))()
        for i, ((cls, tid, _), g) in enumerate(zip(patches, arrs)):
            recs[i] = SbmVerifyPatch(cls, tid, g.shape[1], g.shape[0], g.strides[0] if g.size else g.shape[1], 0, g.ctypes.data)
        _check(lib().sbm_upload_verify_patches(self._h, recs if arrs else None, len(arrs)))

    def upload_verify_patches_raw(self, recs: Sequence[SbmVerifyPatch]):
        """sbm_upload_verify_patches with the caller's own records (any width, height and stride)"""
        arr = (SbmVerifyPatch * max(len(recs), 1))(*recs)
        _check(lib().sbm_upload_verify_patches(self._h, arr, len(recs)))

    def get_verify_patch(self, class_idx: int, template_id: int, width: int, height: int) -> Tuple[np.ndarray, int]:
        """sbm_get_verify_patch: the stored (normalised) patch of a label and the sum of its squares"""
        out = np.zeros((height, width), np.uint8)
        sbb = C.c_uint64(0)
        _check(lib().sbm_get_verify_patch(self._h, class_idx, template_id, _p(out), out.nbytes, C.byref(sbb)))
        return out, int(sbb.value)

    def verify_batch_device(self, d_imgs: int, frame_stride: int, n_frames: int, rows: int, cols: int, stride: int, channels: int,
                            d_recs: int, d_counts: int, cap: int, min_corr: float, d_out: int, d_scores: int, out_cap: int,
                            d_out_counts: int, keep_unverified: bool = False, stream: int = 0):
        """normalised correlation per record against its label's patch (sbm_verify_batch_device): frame f's records at
        d_recs + f*cap records, its {n, overflow} at d_counts + 2*f int32 (sbm_nms_batch_device's output layout); kept records at
        d_out + f*out_cap in input order, scores at d_scores + f*out_cap floats, {n_kept, flags} at d_out_counts + 2*f."""
        prm = SbmVerifyParams(min_corr, int(keep_unverified), 0)
        _check(lib().sbm_verify_batch_device(self._h, C.c_void_p(d_imgs), frame_stride, n_frames, rows, cols, stride, channels,
                                             C.c_void_p(d_recs), C.c_void_p(d_counts), cap, C.byref(prm), C.c_void_p(d_out) if d_out else None,
                                             C.c_void_p(d_scores) if d_scores else None, out_cap, C.c_void_p(d_out_counts),
                                             C.c_void_p(stream) if stream else None))

    def verify_batch_device_ptrs(self, d_frame_ptrs: int, n_frames: int, rows: int, cols: int, stride: int, channels: int, d_recs: int,
                                 d_counts: int, cap: int, min_corr: float, d_out: int, d_scores: int, out_cap: int, d_out_counts: int,
                                 keep_unverified: bool = False, stream: int = 0):
        """verify_batch_device on the frames a device table of addresses names (match_batch_device_ptrs's table)"""
        prm = SbmVerifyParams(min_corr, int(keep_unverified), 0)
        _check(lib().sbm_verify_batch_device_ptrs(self._h, C.c_void_p(d_frame_ptrs) if d_frame_ptrs else None, n_frames, rows, cols, stride,
                                                  channels, C.c_void_p(d_recs), C.c_void_p(d_counts), cap, C.byref(prm),
                                                  C.c_void_p(d_out) if d_out else None, C.c_void_p(d_scores) if d_scores else None, out_cap,
                                                  C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None))

    def verify_batch_device_planes(self, d_plane_ptrs: int, n_frames: int, rows: int, cols: int, stride: int, d_recs: int, d_counts: int,
                                   cap: int, min_corr: float, d_out: int, d_scores: int, out_cap: int, d_out_counts: int,
                                   keep_unverified: bool = False, stream: int = 0):
        """verify_batch_device on planar frames: a device table of 3 plane addresses per frame, B, G, R in the order listed"""
        prm = SbmVerifyParams(min_corr, int(keep_unverified), 0)
        _check(lib().sbm_verify_batch_device_planes(self._h, C.c_void_p(d_plane_ptrs) if d_plane_ptrs else None, n_frames, rows, cols, stride,
                                                    C.c_void_p(d_recs), C.c_void_p(d_counts), cap, C.byref(prm),
                                                    C.c_void_p(d_out) if d_out else None, C.c_void_p(d_scores) if d_scores else None, out_cap,
                                                    C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None))

    def match_batch_host_verified(self, frames: Sequence[np.ndarray], threshold: float, score_threshold: float, nms_threshold: float,
                                  min_corr: float, eta: float = 1.0, top_k: int = 0, keep_unverified: bool = False, cap: int = 1024,
                                  out_cap: int = 256):
        """sbm_match_batch_host_verified: match, NMS and verify on one upload of the frames; per frame the kept records and
        their scores (lists of arrays), and the {n_kept, flags} pairs"""
        arrs = [_img(f) for f in frames]
        r, c, ch = arrs[0][1:]
        assert all(a[1:] == (r, c, ch) for a in arrs)
        ptrs = (C.c_void_p * len(arrs))(*[a[0].ctypes.data for a in arrs])
        out = np.zeros((len(arrs), out_cap), MATCH_DTYPE)
        scores = np.zeros((len(arrs), out_cap), np.float32)
        counts = np.zeros((len(arrs), 2), np.int32)
        nms = SbmNmsParams(score_threshold, nms_threshold, eta, top_k)
        prm = SbmVerifyParams(min_corr, int(keep_unverified), 0)
        _check(lib().sbm_match_batch_host_verified(self._h, ptrs, len(arrs), r, c, c * ch, ch, C.c_float(threshold), cap, C.byref(nms),
                                                   C.byref(prm), _p(out), _p(scores), out_cap, _p(counts)))
        k = [min(int(counts[f, 0]), out_cap) for f in range(len(arrs))]
        return [out[f, : k[f]].copy() for f in range(len(arrs))], [scores[f, : k[f]].copy() for f in range(len(arrs))], counts

    def set_result_mirror(self, mirror_out: int, mirror_count: int):
        """Device-visible (e.g. pinned host) addresses that receive a copy of every result."""
        _check(lib().sbm_set_result_mirror(self._h, C.c_void_p(mirror_out) if mirror_out else None,
                                           C.c_void_p(mirror_count) if mirror_count else None))

    # -- multi-GPU exchange (RCCL inside the library) -------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(lib().sbm_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, world: int, rank: int, uid: bytes):
        assert len(uid) == 128
        _check(lib().sbm_comm_init(self._h, world, rank, C.c_char_p(uid)))

    def comm_count(self) -> int:
        """ranks of this context's communicator as RCCL reports them (ncclCommCount)"""
        n = C.c_int32(0)
        _check(lib().sbm_comm_count(self._h, C.byref(n)))
        return int(n.value)

    def match_templates_device_sharded(self, threshold: float, d_local: int, cap: int, d_gathered: int, gathered_mirror: int = 0,
                                       stream: int = 0):
        _check(lib().sbm_match_templates_device_sharded(self._h, C.c_float(threshold), C.c_void_p(d_local), cap, C.c_void_p(d_gathered),
                                                        C.c_void_p(gathered_mirror) if gathered_mirror else None,
                                                        C.c_void_p(stream) if stream else None))

    def match_device_sharded(self, d_img: int, rows: int, cols: int, stride: int, channels: int, threshold: float,
                             d_local: int, cap: int, d_gathered: int, gathered_mirror: int = 0, stream: int = 0,
                             d_mask: int = 0):
        _check(lib().sbm_match_device_sharded(self._h, C.c_void_p(d_img), rows, cols, stride, channels,
                                              C.c_void_p(d_mask) if d_mask else None, C.c_float(threshold),
                                              C.c_void_p(d_local), cap, C.c_void_p(d_gathered),
                                              C.c_void_p(gathered_mirror) if gathered_mirror else None,
                                              C.c_void_p(stream) if stream else None))

    def match_batch_device_sharded(self, d_imgs: int, frame_stride: int, n_frames: int, rows: int, cols: int, stride: int,
                                   channels: int, threshold: float, d_local: int, cap: int, d_gathered: int,
                                   gathered_mirror: int = 0, stream: int = 0, d_mask: int = 0):
        _check(lib().sbm_match_batch_device_sharded(self._h, C.c_void_p(d_imgs), frame_stride, n_frames, rows, cols, stride,
                                                    channels, C.c_void_p(d_mask) if d_mask else None, C.c_float(threshold),
                                                    C.c_void_p(d_local), cap, C.c_void_p(d_gathered),
                                                    C.c_void_p(gathered_mirror) if gathered_mirror else None,
                                                    C.c_void_p(stream) if stream else None))

    def match_batch_device_banded(self, d_imgs: int, frame_stride: int, n_frames: int, rows: int, cols: int, stride: int,
                                  channels: int, threshold: float, d_local: int, cap: int, d_gathered: int = 0,
                                  gathered_mirror: int = 0, n_bands: int = 0, stream: int = 0, d_mask: int = 0):
        """build-sharded step: this rank's row band of every level's orientation map, grouped in-place all-gather of the
        bands, linear memories, template loop, gather of the match lists (one GPU: all n_bands bands, one launch each)"""
        _check(lib().sbm_match_batch_device_banded(self._h, C.c_void_p(d_imgs), frame_stride, n_frames, rows, cols, stride,
                                                   channels, C.c_void_p(d_mask) if d_mask else None, C.c_float(threshold),
                                                   C.c_void_p(d_local), cap, C.c_void_p(d_gathered) if d_gathered else None,
                                                   C.c_void_p(gathered_mirror) if gathered_mirror else None, n_bands,
                                                   C.c_void_p(stream) if stream else None))

    def extract_local_maxima(self, magnitude: np.ndarray, strong_threshold: float, mask: Optional[np.ndarray] = None) -> np.ndarray:
        """[(x, y)] of the 5x5 local maxima extractTemplate accepts (row-major order)"""
        mag = np.ascontiguousarray(magnitude, np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        cap = max(16, mag.size // 4)
        xy = np.zeros(cap, np.int32)
        n = C.c_int64(0)
        _check(lib().sbm_extract_local_maxima(self._h, _p(mag), _p(m), mag.shape[0], mag.shape[1], C.c_float(strong_threshold), _p(xy), cap,
                                              C.byref(n)))
        xy = xy[: n.value]
        return np.stack([xy & 0xFFFF, xy >> 16], axis=1)

    def train_batch_device(self, d_imgs: int, img_stride: int, n_images: int, rows: int, cols: int, stride: int, channels: int,
                           strong_threshold: float, num_features: int, d_levels: int, d_feats: int, feat_cap: int, d_status: int,
                           stream: int = 0, d_masks: int = 0, mask_stride: int = 0):
        """Detector::addTemplate for n_images images of one geometry, on the device (sbm_train_batch_device): image i at
        d_imgs + i*img_stride; its n_levels level records at d_levels, its features at d_feats + i*feat_cap records, its
        {status, count} at d_status + 2*i int32.  d_masks 0: no mask; mask_stride 0: one mask for all images."""
        _check(lib().sbm_train_batch_device(self._h, C.c_void_p(d_imgs), img_stride, n_images, rows, cols, stride, channels,
                                            C.c_void_p(d_masks) if d_masks else None, mask_stride, C.c_float(strong_threshold),
                                            num_features, C.c_void_p(d_levels), C.c_void_p(d_feats) if d_feats else None, feat_cap,
                                            C.c_void_p(d_status), C.c_void_p(stream) if stream else None))

    def train_batch_raw(self, imgs: Sequence[np.ndarray], masks: Optional[Sequence[Optional[np.ndarray]]], strong_threshold: float,
                        num_features: int, feat_cap: int):
        """sbm_train_batch as it is: (levels[n, n_levels], feats[n, feat_cap], status[n, 2])"""
        arrs = [_img(im) for im in imgs]
        if not arrs:
            raise ValueError("no images")
        _, r, c, ch = arrs[0]
        if any(a[1:] != (r, c, ch) for a in arrs):
            raise ValueError("the images of a batch share one geometry")
        n = len(arrs)
        ms = [None] * n if masks is None else [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
        if len(ms) != n or any(m is not None and m.shape != (r, c) for m in ms):
            raise ValueError("masks: None, or one (rows, cols) array or None per image")
        ip = (C.c_void_p * n)(*[a[0].ctypes.data for a in arrs])
        mp = (C.c_void_p * n)(*[None if m is None else m.ctypes.data for m in ms])
        levels = np.zeros((n, self.n_levels), LEVEL_DTYPE)
        feats = np.zeros((n, max(feat_cap, 1)), TRAIN_FEATURE_DTYPE)
        status = np.zeros((n, 2), np.int32)
        _check(lib().sbm_train_batch(self._h, ip, n, r, c, c * ch, ch, None if masks is None else mp, C.c_float(strong_threshold), num_features,
                                     _p(levels), _p(feats), feat_cap, _p(status)))
        return levels, feats[:, :feat_cap], status

    def train_batch(self, imgs: Sequence[np.ndarray], masks: Optional[Sequence[Optional[np.ndarray]]], strong: float, num_features: int):
        """Detector::addTemplate for every image of a batch of one geometry: a list of (levels, feats), None where
        addTemplate returns -1.  masks: None, or per image a (rows, cols) array or None."""
        _, r, c, _ = _img(imgs[0])
        cap = sum(((r >> l) + 2) // 3 * (((c >> l) + 2) // 3) for l in range(self.n_levels))  # no more maxima than 3x3 cells
        levels, feats, status = self.train_batch_raw(imgs, masks, strong, num_features, cap)
        out = []
        for i in range(len(imgs)):
            if status[i, 0] == 1:
                out.append(None)
                continue
            if status[i, 0] != 0:
                raise SbmError(-3, f"image {i}: {status[i, 1]} features exceed the capacity {cap}")
            out.append((levels[i].copy(), feats[i, : status[i, 1]].copy()))
        return out

    # ---- ragged batched training: images of different sizes and feature counts in one call --------------------------
    def _feature_cap(self, rows: int, cols: int) -> int:
        """no more accepted maxima than 3 x 3 cells, level by level: the most features an image can have"""
        return sum(((rows >> l) + 2) // 3 * (((cols >> l) + 2) // 3) for l in range(self.n_levels))

    def train_ragged_device(self, images: Sequence["SbmTrainImage"], channels: int, strong_threshold: float, d_levels: int, d_feats: int,
                            d_status: int, stream: int = 0):
        """sbm_train_ragged_device: `images` are descriptors of device images (read during the call only); image i's
        n_levels level records at d_levels, its features in its own block of d_feats, {status, count} at d_status + 2*i."""
        arr = (SbmTrainImage * max(len(images), 1))(*images)
        _check(lib().sbm_train_ragged_device(self._h, arr, len(images), channels, C.c_float(strong_threshold), C.c_void_p(d_levels),
                                             C.c_void_p(d_feats) if d_feats else None, C.c_void_p(d_status),
                                             C.c_void_p(stream) if stream else None))

    def train_ragged_raw(self, imgs: Sequence[np.ndarray], masks: Optional[Sequence[Optional[np.ndarray]]], strong_threshold: float,
                         num_features_each: Sequence[int], feat_caps: Sequence[int], feat_firsts: Optional[Sequence[int]] = None,
                         feats: Optional[np.ndarray] = None):
        """sbm_train_ragged as it is: (levels[n, n_levels], feats[total], status[n, 2], firsts[n]).  Image i's block of
        feat_caps[i] records starts at feat_firsts[i] (None: the blocks behind each other); `feats`, if given, is the
        feature array the call writes into (a caller's fill stays where no block lies)."""
        arrs = [_img(im) for im in imgs]
        n = len(arrs)
        ch = arrs[0][3] if arrs else 3
        if any(a[3] != ch for a in arrs):
            raise ValueError("the images of a call share the number of channels")
        ms = [None] * n if masks is None else [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
        if len(ms) != n or any(m is not None and m.shape != (a[1], a[2]) for m, a in zip(ms, arrs)):
            raise ValueError("masks: None, or one (rows, cols) array or None per image")
        if len(num_features_each) != n or len(feat_caps) != n:
            raise ValueError("one feature count and one capacity per image")
        firsts = list(np.cumsum([0] + [max(int(c), 0) for c in feat_caps])[:-1]) if feat_firsts is None else list(feat_firsts)
        desc = (SbmTrainImage * max(n, 1))()
        for i, (a, r, c, _) in enumerate(arrs):
            desc[i] = SbmTrainImage(a.ctypes.data, None if ms[i] is None else ms[i].ctypes.data, r, c, c * ch, int(num_features_each[i]),
                                    int(firsts[i]), int(feat_caps[i]))
        end = max([int(f) + max(int(c), 0) for f, c in zip(firsts, feat_caps)] + [0])
        if feats is None:
            feats = np.zeros(max(end, 1), TRAIN_FEATURE_DTYPE)
        levels = np.zeros((n, self.n_levels), LEVEL_DTYPE)
        status = np.zeros((n, 2), np.int32)
        _check(lib().sbm_train_ragged(self._h, desc, n, ch, C.c_float(strong_threshold), _p(levels), _p(feats), _p(status)))
        return levels, feats, status, firsts

    @staticmethod
    def _train_results(levels, feats, status, firsts, caps):
        out = []
        for i in range(len(levels)):
            if status[i, 0] == 1:
                out.append(None)
                continue
            if status[i, 0] != 0:
                raise SbmError(-3, f"image {i}: {status[i, 1]} features exceed the capacity {caps[i]}")
            out.append((levels[i].copy(), feats[firsts[i]: firsts[i] + status[i, 1]].copy()))
        return out

    def train_ragged_status(self, imgs: Sequence[np.ndarray], masks: Optional[Sequence[Optional[np.ndarray]]], strong: float,
                            num_features_each: Sequence[int]):
        """train_ragged and the status array [n, 2]: {0, features} | {1, first failing level}"""
        caps = [self._feature_cap(*_img(im)[1:3]) for im in imgs]
        levels, feats, status, firsts = self.train_ragged_raw(imgs, masks, strong, num_features_each, caps)
        return self._train_results(levels, feats, status, firsts, caps), status

    def train_ragged(self, imgs: Sequence[np.ndarray], masks: Optional[Sequence[Optional[np.ndarray]]], strong: float,
                     num_features_each: Sequence[int]):
        """Detector::addTemplate(imgs[i], masks[i], num_features_each[i]) for images of any sizes in one call: a list of
        (levels, feats), None where addTemplate returns -1 (an image too small for the pyramid included)."""
        return self.train_ragged_status(imgs, masks, strong, num_features_each)[0]

    def sweep_dims(self, rows: int, cols: int, fx: float, fy: float):
        """the size cv::resize(img, Size(), fx, fy) gives a rows x cols image (sbm_resize_linear's size query)"""
        dr, dc = C.c_int32(0), C.c_int32(0)
        probe = np.zeros(1, np.uint8)
        _check(lib().sbm_resize_linear(self._h, _p(probe), rows, cols, cols, 1, fx, fy, None, 0, C.byref(dr), C.byref(dc)))
        return dr.value, dc.value

    def train_sweep_status(self, img: np.ndarray, mask: Optional[np.ndarray], scales: Sequence[float], strong: float,
                           num_features_each: Sequence[int]):
        """train_sweep and the status array [n, 2].  A scale is a number (fx = fy) or a pair (fx, fy)."""
        a, r, c, ch = _img(img)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != (r, c):
            raise ValueError("mask: a (rows, cols) array")
        n = len(scales)
        if len(num_features_each) != n:
            raise ValueError("one feature count per scale")
        fxy = [(float(s[0]), float(s[1])) if isinstance(s, (tuple, list)) else (float(s), float(s)) for s in scales]
        desc = (SbmTrainScale * max(n, 1))()
        caps, firsts, first = [], [], 0
        for k, (fx, fy) in enumerate(fxy):
            dr, dc = self.sweep_dims(r, c, fx, fy)
            caps.append(self._feature_cap(max(dr, 0), max(dc, 0)))
            firsts.append(first)
            desc[k] = SbmTrainScale(fx, fy, int(num_features_each[k]), 0, first, caps[k])
            first += caps[k]
        levels = np.zeros((n, self.n_levels), LEVEL_DTYPE)
        feats = np.zeros(max(first, 1), TRAIN_FEATURE_DTYPE)
        status = np.zeros((n, 2), np.int32)
        _check(lib().sbm_train_sweep(self._h, _p(a), r, c, c * ch, ch, _p(m), desc, n, C.c_float(strong), _p(levels), _p(feats), _p(status)))
        return self._train_results(levels, feats, status, firsts, caps), status

    def train_sweep(self, img: np.ndarray, mask: Optional[np.ndarray], scales: Sequence[float], strong: float, num_features_each: Sequence[int]):
        """The scale sweep of shapeInfo_producer: Detector::addTemplate(resize(img, s), resize(mask, s) > 0,
        num_features_each[k]) for every scale s, the source uploaded once and resized on the device: a list of
        (levels, feats), None where addTemplate returns -1."""
        return self.train_sweep_status(img, mask, scales, strong, num_features_each)[0]

    # ---- rotated template families: Detector::addTemplate_rotate for every (base, angle) pair of a call ----------------
    def train_rotate_device(self, bases: Sequence["SbmRotateBase"], thetas: Sequence[float], d_levels: int, d_feats: int, d_status: int,
                            stream: int = 0):
        """sbm_train_rotate_device: `bases` are records of device addresses (read during the call only, as `thetas`); pair
        p = b * len(thetas) + k writes its n_levels level records at d_levels, its features in rotation k's block of base
        b, {status, value} at d_status + 2*p."""
        arr = (SbmRotateBase * max(len(bases), 1))(*bases)
        th = np.ascontiguousarray(thetas, np.float32)
        _check(lib().sbm_train_rotate_device(self._h, arr, len(bases), _p(th), len(th), C.c_void_p(d_levels),
                                             C.c_void_p(d_feats) if d_feats else None, C.c_void_p(d_status),
                                             C.c_void_p(stream) if stream else None))

    def train_rotate_raw(self, bases, thetas: Sequence[float], centers, out_caps: Sequence[int], out_firsts: Optional[Sequence[int]] = None,
                         feats: Optional[np.ndarray] = None):
        """sbm_train_rotate as it is: (levels[n_bases, n_thetas, n_levels], feats[total], status[n_bases, n_thetas, 2],
        firsts[n_bases]).  A base is (levels, feats) or (levels, feats, status pair); rotation k of base b has the block of
        out_caps[b] records from out_firsts[b] + k * out_caps[b] (None: the bases' blocks behind each other); `feats`, if
        given, is the feature array the call writes into (a caller's fill stays where no pair that is ok writes)."""
        nb, th = len(bases), np.ascontiguousarray(thetas, np.float32)
        nt = len(th)
        if len(centers) != nb or len(out_caps) != nb:
            raise ValueError("one centre and one capacity per base")
        firsts = list(np.cumsum([0] + [max(int(c), 0) * nt for c in out_caps])[:-1]) if out_firsts is None else list(out_firsts)
        keep, desc = [], (SbmRotateBase * max(nb, 1))()
        for b, base in enumerate(bases):
            lv = np.ascontiguousarray(base[0], LEVEL_DTYPE)
            ft = np.ascontiguousarray(base[1], TRAIN_FEATURE_DTYPE)
            if len(ft) == 0:
                ft = np.zeros(1, TRAIN_FEATURE_DTYPE)
            st = None if len(base) < 3 or base[2] is None else np.ascontiguousarray(base[2], np.int32)
            if len(lv) != self.n_levels or (st is not None and st.shape != (2,)):
                raise ValueError("a base: n_levels level records, its features, and None or a status pair")
            keep.append((lv, ft, st))
            desc[b] = SbmRotateBase(lv.ctypes.data, ft.ctypes.data, None if st is None else st.ctypes.data, float(centers[b][0]), float(centers[b][1]),
                                    int(firsts[b]), int(out_caps[b]))
        end = max([int(f) + max(int(c), 0) * nt for f, c in zip(firsts, out_caps)] + [0])
        if feats is None:
            feats = np.zeros(max(end, 1), TRAIN_FEATURE_DTYPE)
        levels = np.zeros((nb, max(nt, 1), self.n_levels), LEVEL_DTYPE)
        status = np.zeros((nb, max(nt, 1), 2), np.int32)
        _check(lib().sbm_train_rotate(self._h, desc, nb, _p(th), nt, _p(levels), _p(feats), _p(status)))
        return levels, feats, status, firsts

    def train_rotate(self, bases, thetas: Sequence[float], centers):
        """Detector::addTemplate_rotate(class, base b, thetas[k], centers[b]) for every base and angle in one call.  A base
        is (levels, feats) as the train_* calls return it, or None (a template whose training failed).  Returns a list over
        the pairs p = b * len(thetas) + k of (levels, feats), None for the pairs of a base that is None."""
        zero = np.zeros(self.n_levels, LEVEL_DTYPE)
        failed = np.array([1, 0], np.int32)
        full = [(zero, np.zeros(1, TRAIN_FEATURE_DTYPE), failed) if b is None else (b[0], b[1], None) for b in bases]
        caps = [0 if b is None else max(int(np.asarray(b[0]["n_features"]).clip(0).sum()), 1) for b in bases]
        levels, feats, status, firsts = self.train_rotate_raw(full, thetas, centers, caps)
        out = []
        for b in range(len(bases)):
            for k in range(len(thetas)):
                code, value = int(status[b, k, 0]), int(status[b, k, 1])
                if code == 1:
                    out.append(None)
                    continue
                if code != 0:
                    raise SbmError(-3, f"base {b}, angle {k}: status {{{code}, {value}}}")
                first = firsts[b] + k * caps[b]
                out.append((levels[b, k].copy(), feats[first: first + value].copy()))
        return out

    def select_templates(self, idx: Sequence[int]):
        a = np.ascontiguousarray(idx, np.int32)
        _check(lib().sbm_select_templates(self._h, _p(a), len(a)))

    def partition_templates(self, rows: int, cols: int, n_shards: int, idx: Optional[Sequence[int]] = None):
        """work-balanced contiguous shards [(first, count)] of the template list ``idx`` (None: all, upload order)"""
        a = None if idx is None else np.ascontiguousarray(idx, np.int32)
        first = np.zeros(n_shards, np.int32)
        count = np.zeros(n_shards, np.int32)
        _check(lib().sbm_partition_templates(self._h, rows, cols, _p(a), 0 if a is None else len(a), n_shards, _p(first), _p(count)))
        return list(zip(first.tolist(), count.tolist()))

    @staticmethod
    def match_sharded(ctxs: Sequence["Context"], img: np.ndarray, threshold: float, mask: Optional[np.ndarray] = None,
                      cap: int = 1 << 16) -> np.ndarray:
        """single-process multi-GPU match: one context (and host thread) per GPU, lists concatenated on the host"""
        img, r, c, ch = _img(img)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        hs = (C.c_void_p * len(ctxs))(*[x._h for x in ctxs])
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_int64(0)
        _check(lib().sbm_match_sharded(hs, len(ctxs), _p(img), r, c, c * ch, ch, _p(m), C.c_float(threshold), _p(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def match_batch_host(self, frames: Sequence[np.ndarray], threshold: float, cap: int = 1024, sub_batch: int = 0,
                         mask: Optional[np.ndarray] = None, split: bool = False):
        """frames in host memory, pipelined uploads; returns a list of record arrays (one per frame).
        split=True: sbm_match_batch_host_begin, then _end (the asynchronous form)"""
        arrs = [_img(f) for f in frames]
        r, c, ch = arrs[0][1:]
        assert all(a[1:] == (r, c, ch) for a in arrs)
        ptrs = (C.c_void_p * len(arrs))(*[a[0].ctypes.data for a in arrs])
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.zeros((len(arrs), cap), MATCH_DTYPE)
        counts = np.zeros((len(arrs), 2), np.int32)
        if split:
            _check(lib().sbm_match_batch_host_begin(self._h, ptrs, len(arrs), r, c, c * ch, ch, _p(m), C.c_float(threshold), cap, sub_batch))
            _check(lib().sbm_match_batch_host_end(self._h, _p(out), _p(counts)))
        else:
            _check(lib().sbm_match_batch_host(self._h, ptrs, len(arrs), r, c, c * ch, ch, _p(m), C.c_float(threshold), _p(out), cap,
                                              _p(counts), sub_batch))
        return [out[f, : counts[f, 0]].copy() for f in range(len(arrs))]

    def match_batch_host_masked(self, frames: Sequence[np.ndarray], masks: Sequence[Optional[np.ndarray]], threshold: float,
                                cap: int = 1024, sub_batch: int = 0, split: bool = False, nms: Optional[SbmNmsParams] = None,
                                out_cap: int = 256):
        """match_batch_host with one mask per frame (None: no mask for that frame).  Arrays that are already contiguous
        uint8 are passed as they are (pinned ones stay pinned).  nms: end with sbm_match_batch_host_end_nms instead and
        return (kept lists, {n_kept, flags} pairs)."""
        arrs = [_img(f) for f in frames]
        r, c, ch = arrs[0][1:]
        assert all(a[1:] == (r, c, ch) for a in arrs) and len(masks) == len(arrs)
        ms = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
        assert all(m is None or m.shape == (r, c) for m in ms)
        ptrs = (C.c_void_p * len(arrs))(*[a[0].ctypes.data for a in arrs])
        mptrs = (C.c_void_p * len(arrs))(*[None if m is None else m.ctypes.data for m in ms])
        counts = np.zeros((len(arrs), 2), np.int32)
        if nms is not None:
            out = np.zeros((len(arrs), out_cap), MATCH_DTYPE)
            _check(lib().sbm_match_batch_host_begin_masked(self._h, ptrs, len(arrs), r, c, c * ch, ch, mptrs, C.c_float(threshold), cap, sub_batch))
            _check(lib().sbm_match_batch_host_end_nms(self._h, C.byref(nms), _p(out), out_cap, _p(counts)))
            return [out[f, : counts[f, 0]].copy() for f in range(len(arrs))], counts
        out = np.zeros((len(arrs), cap), MATCH_DTYPE)
        if split:
            _check(lib().sbm_match_batch_host_begin_masked(self._h, ptrs, len(arrs), r, c, c * ch, ch, mptrs, C.c_float(threshold), cap, sub_batch))
            _check(lib().sbm_match_batch_host_end(self._h, _p(out), _p(counts)))
        else:
            _check(lib().sbm_match_batch_host_masked(self._h, ptrs, len(arrs), r, c, c * ch, ch, mptrs, C.c_float(threshold), _p(out), cap,
                                                     _p(counts), sub_batch))
        return [out[f, : counts[f, 0]].copy() for f in range(len(arrs))]

    def pin_host_buffer(self, a: np.ndarray):
        """explicit opt-in: frames inside ``a`` are uploaded by direct DMA until unpin_host_buffer(a) / close()"""
        _check(lib().sbm_pin_host_buffer(self._h, C.c_void_p(a.ctypes.data), a.nbytes))

    def unpin_host_buffer(self, a: np.ndarray):
        _check(lib().sbm_unpin_host_buffer(self._h, C.c_void_p(a.ctypes.data)))

    def set_quantize_mode(self, mode: str = "auto", rows_per_wave: int = 0):
        """gradient kernel choice: "auto" (by launch size), "tile" or "stream"; bit-identical results"""
        _check(lib().sbm_set_quantize_mode(self._h, {"auto": 0, "tile": 1, "stream": 2}[mode], rows_per_wave))

    def set_coarse_mode(self, mode: str = "auto"):
        """coarse-pass kernel: "auto" (bit planes whenever the threshold is >= 0), "block" (bytes, four waves per item), "wave"
        (bytes, one wave per item), "bits", "bytes" (block or wave by launch size); identical candidates"""
        _check(lib().sbm_set_coarse_mode(self._h, {"auto": 0, "": 0, "block": 1, "wave": 2, "bits": 3, "bytes": 4}[mode]))

    def set_refine_bits(self, mode=None):
        """None: the process default; True: T = 4 refinement levels as bit strips; False: as spread bytes (sbm.h)."""
        _check(lib().sbm_set_refine_bits(self._h, -1 if mode is None else (1 if mode else 0)))

    def set_refine_order(self, order: str = "auto"):
        """refinement pass: "auto" (by the batch's plane size), "slots" (per-frame slots) or "list" (one frame-major list)"""
        _check(lib().sbm_set_refine_order(self._h, {"auto": -1, "slots": 0, "list": 2}[order]))

    def set_pipeline_depth(self, batches_in_flight: int):
        """hint: the caller keeps this many batches in flight on the GPU -> launches are sized for throughput (>= 2)"""
        _check(lib().sbm_set_pipeline_depth(self._h, batches_in_flight))

    def set_sparse_list_rows(self, rows_per_item: int = -1):
        """rows per work item of the grid the lists of working items of the sparse level-0 gradient launch are made on: -1 the
        process default, 0 the launch's own rows per item, > 0 that many (sbm.h); identical results"""
        _check(lib().sbm_set_sparse_list_rows(self._h, rows_per_item))

    def graph_count(self) -> int:
        n = C.c_int32(0)
        _check(lib().sbm_graph_count(self._h, C.byref(n)))
        return int(n.value)

    def set_graph_mode(self, on):
        """True: always replay captured hipGraphs; False: never; None / "auto" (the library's default): batch and template-loop
        entry points replay once several calls are in flight (set_pipeline_depth >= 2) and an argument tuple repeats"""
        _check(lib().sbm_set_graph_mode(self._h, -1 if on is None or on == "auto" else (1 if on else 0)))

    # -- pyramid state ------------------------------------------------------------
    def build_pyramid(self, img: np.ndarray, mask: Optional[np.ndarray] = None):
        img, r, c, ch = _img(img)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        _check(lib().sbm_build_pyramid(self._h, _p(img), r, c, c * ch, ch, _p(m)))

    def set_quantized(self, level: int, q: np.ndarray):
        q = np.ascontiguousarray(q, np.uint8)
        _check(lib().sbm_set_quantized(self._h, level, _p(q), q.shape[0], q.shape[1]))

    def level_dims(self, level: int) -> Tuple[int, int]:
        r, c = C.c_int32(), C.c_int32()
        _check(lib().sbm_level_dims(self._h, level, C.byref(r), C.byref(c)))
        return r.value, c.value

    def get_quantized(self, level: int) -> np.ndarray:
        r, c = self.level_dims(level)
        out = np.empty((r, c), np.uint8)
        _check(lib().sbm_get_quantized(self._h, level, _p(out)))
        return out

    def get_quantized_frame(self, level: int, frame: int) -> np.ndarray:
        """the one-hot orientation map of frame ``frame`` of the last batch at ``level``"""
        r, c = self.level_dims(level)
        out = np.empty((r, c), np.uint8)
        _check(lib().sbm_get_quantized_frame(self._h, level, frame, _p(out)))
        return out

    def get_linear_memories(self, level: int) -> np.ndarray:
        s = C.c_int64()
        _check(lib().sbm_get_linear_memories(self._h, level, None, 0, C.byref(s)))
        out = np.empty((8, s.value), np.uint8)
        _check(lib().sbm_get_linear_memories(self._h, level, _p(out), out.nbytes, C.byref(s)))
        return out

    def get_coarse_bitplanes(self, frame: int = 0) -> np.ndarray:
        """[16][lm_stride / 8] bytes: the coarsest level's "response > 0" (0..7) and "response == 4" (8..15) bit planes"""
        s = C.c_int64()
        _check(lib().sbm_get_linear_memories(self._h, self.n_levels - 1, None, 0, C.byref(s)))
        out = np.empty((16, s.value // 8), np.uint8)
        _check(lib().sbm_get_coarse_bitplanes(self._h, frame, _p(out), out.nbytes))
        return out

    def coarse_form(self) -> Tuple[int, int, int, int]:
        """(kind, P, wide, dw) of the coarse kernel the last call launched: kind 0 none yet, 1 bytes with four waves per item,
        2 bytes with one wave per item, 3 bit planes with one wave per item, 4 bit planes with eight waves per item"""
        out = np.zeros(4, np.int32)
        _check(lib().sbm_get_coarse_form(self._h, _p(out)))
        return tuple(int(v) for v in out)

    def refine_form(self, level: int = 0) -> Tuple[int, int, int, int, int, int]:
        """(kind, LW, order, t8, sparse, slots) of the refinement kernel the last call launched at ``level``: kind 0 none yet,
        1 the 8 response planes, 2 the spread plane row-major, 3 the spread plane in strips, 4 bit strips"""
        out = np.zeros(6, np.int32)
        _check(lib().sbm_get_refine_form(self._h, level, _p(out)))
        return tuple(int(v) for v in out)

    def source_form(self) -> int:
        """the source pass of the last call: 0 none (level 0's map was built whole), 1 the strided form, 2 the line-shaped kernel"""
        out = C.c_int32(0)
        _check(lib().sbm_get_source_form(self._h, C.byref(out)))
        return int(out.value)

    def source_retention(self) -> Tuple[int, int]:
        """(retained, skipped): the calls of this context whose source pass stored the retained copy of level 0's source, and
        those whose source pass left it unwritten because a later call was already enqueued behind them; waits for the device"""
        out = np.zeros(2, np.int32)
        _check(lib().sbm_get_source_retention(self._h, _p(out)))
        return tuple(int(v) for v in out)

    def sparse_items(self) -> Tuple[int, int, int]:
        """(selection, working, launched) of the last call's sparse level-0 gradient launch: selection 0 none, 1 by tile flags,
        2 by the record of need rectangles; working items are counted under profiling only (-1 otherwise)"""
        out = np.zeros(3, np.int32)
        _check(lib().sbm_get_sparse_items(self._h, _p(out)))
        return tuple(int(v) for v in out)

    def sparse_list(self) -> Tuple[int, int]:
        """(list_mode, slots_per_frame) of the last call's sparse level-0 gradient launch: list_mode 1 when it ran from the lists
        of working items, with slots_per_frame waves per frame; (0, 0) otherwise"""
        out = np.zeros(3, np.int32)
        _check(lib().sbm_get_sparse_list(self._h, _p(out)))
        return tuple(int(v) for v in out[:2])

    def sparse_list_rows(self) -> int:
        """rows per work item of the grid the last call's lists of working items were made on (the third value of
        sbm_get_sparse_list): what a listed frame's items have in the sparse level-0 gradient launch; 0 when it ran from no lists"""
        out = np.zeros(3, np.int32)
        _check(lib().sbm_get_sparse_list(self._h, _p(out)))
        return int(out[2])

    def level_build(self, level: int) -> Tuple[int, int, int, int, int, int]:
        """(current, form, builder, split, allty, packed) of ``level``: the buffers that are current as the bit set planes8 1,
        spread 2, strip 4, bit strips 8, bit planes 16; the LmForm of its last build (5: sparse bit strips); the builder 0 none,
        1 k_build_lm_rows, 2 k_build_lm_any, 3 k_build_lm, 4 the unfused path; split and allty of that launch; packed 1 when
        the bit planes came from k_pack_bitplanes_spread, 2 from k_pack_bitplanes, else 0"""
        out = np.zeros(6, np.int32)
        _check(lib().sbm_get_level_build(self._h, level, _p(out)))
        return tuple(int(v) for v in out)

    def level_stored(self, level: int, frame: int, which: int) -> np.ndarray:
        """the bytes of frame ``frame``'s whole share of one buffer of ``level``, tail included, as they lie in device memory:
        ``which`` 0 the 8 response planes, 1 the spread plane, 2 the bit strips, 3 the refinement-tile flags (level 0)"""
        n = C.c_int64(0)
        _check(lib().sbm_get_level_stored(self._h, level, frame, which, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        _check(lib().sbm_get_level_stored(self._h, level, frame, which, _p(out), out.nbytes, C.byref(n)))
        return out

    def match_templates(self, threshold: float) -> np.ndarray:
        out = np.empty(self._cap, MATCH_DTYPE)
        n = C.c_int64(0)
        _check(lib().sbm_match_templates(self._h, C.c_float(threshold), _p(out), self._cap, C.byref(n)))
        return out[: n.value].copy()

    def match_templates_device(self, threshold: float, d_out: int, cap: int, d_count: int, stream: int = 0):
        _check(lib().sbm_match_templates_device(self._h, C.c_float(threshold), C.c_void_p(d_out), cap, C.c_void_p(d_count),
                                                C.c_void_p(stream) if stream else None))

    # -- single reference functions -------------------------------------------
    def quantized_orientations(self, img: np.ndarray, weak: float, want_float: bool = True):
        img, r, c, ch = _img(img)
        ang = np.empty((r, c), np.uint8)
        mag = np.empty((r, c), np.float32) if want_float else None
        ori = np.empty((r, c), np.float32) if want_float else None
        _check(lib().sbm_quantized_orientations(self._h, _p(img), r, c, c * ch, ch, C.c_float(weak), _p(mag), _p(ang), _p(ori)))
        return mag, ang, ori

    def orientation_bins(self, gx: np.ndarray, gy: np.ndarray) -> np.ndarray:
        gx = np.ascontiguousarray(gx, np.int16)
        gy = np.ascontiguousarray(gy, np.int16)
        out = np.empty(gx.shape, np.uint8)
        _check(lib().sbm_orientation_bins(self._h, _p(gx), _p(gy), gx.size, _p(out)))
        return out

    def pyrdown(self, img: np.ndarray) -> np.ndarray:
        img, r, c, ch = _img(img)
        shape = (r // 2, c // 2) if img.ndim == 2 else (r // 2, c // 2, ch)
        out = np.empty(shape, np.uint8)
        _check(lib().sbm_pyrdown(self._h, _p(img), r, c, c * ch, ch, _p(out)))
        return out

    def resize_linear(self, img: np.ndarray, fx: float, fy: float) -> np.ndarray:
        """cv::resize(img, Size(), fx, fy, INTER_LINEAR) of an 8-bit image (shapeInfo_producer::transform)"""
        a, r, c, ch = _img(img)
        dr, dc = C.c_int32(0), C.c_int32(0)
        _check(lib().sbm_resize_linear(self._h, _p(a), r, c, c * ch, ch, fx, fy, None, 0, C.byref(dr), C.byref(dc)))
        out = np.empty((dr.value, dc.value) if a.ndim == 2 else (dr.value, dc.value, ch), np.uint8)
        _check(lib().sbm_resize_linear(self._h, _p(a), r, c, c * ch, ch, fx, fy, _p(out), out.size, C.byref(dr), C.byref(dc)))
        return out

    def spread(self, q: np.ndarray, T: int) -> np.ndarray:
        q = np.ascontiguousarray(q, np.uint8)
        out = np.empty_like(q)
        _check(lib().sbm_spread(self._h, _p(q), q.shape[0], q.shape[1], T, _p(out)))
        return out

    def compute_response_maps(self, sp: np.ndarray) -> np.ndarray:
        sp = np.ascontiguousarray(sp, np.uint8)
        out = np.empty((8,) + sp.shape, np.uint8)
        _check(lib().sbm_compute_response_maps(self._h, _p(sp), sp.shape[0], sp.shape[1], _p(out)))
        return out

    def linearize(self, m: np.ndarray, T: int) -> np.ndarray:
        m = np.ascontiguousarray(m, np.uint8)
        r, c = m.shape
        out = np.empty((T * T, (r // T) * (c // T)), np.uint8)
        _check(lib().sbm_linearize(self._h, _p(m), r, c, T, _p(out)))
        return out

    def similarity(self, template_index: int) -> np.ndarray:
        lc = self.n_levels - 1
        r, c = self.level_dims(lc)
        T = self.T[lc]
        out = np.empty((r // T, c // T), np.uint16)
        _check(lib().sbm_similarity(self._h, template_index, _p(out)))
        return out

    def similarity_local(self, level: int, template_index: int, cx: int, cy: int) -> np.ndarray:
        out = np.empty((16, 16), np.uint16)
        _check(lib().sbm_similarity_local(self._h, level, template_index, cx, cy, _p(out)))
        return out

    # -- measurement -----------------------------------------------------------
    def set_profiling(self, on: bool, accumulate: bool = False):
        """accumulate: timings of successive asynchronous calls pile up until timings() reads them"""
        _check(lib().sbm_set_profiling(self._h, (2 if accumulate else 1) if on else 0))

    def timings(self) -> List[Tuple[str, float]]:
        n = C.c_int32(0)
        _check(lib().sbm_get_timings(self._h, None, None, 0, C.byref(n)))
        names = (C.c_char_p * max(n.value, 1))()
        ms = (C.c_float * max(n.value, 1))()
        _check(lib().sbm_get_timings(self._h, names, ms, n.value, C.byref(n)))
        return [(names[i].decode(), float(ms[i])) for i in range(n.value)]

    def stats(self) -> Tuple[int, int]:
        """(coarse candidates, refinement bytes) of the last template-matching call."""
        a, b = C.c_int64(0), C.c_int64(0)
        _check(lib().sbm_get_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def coarse_bytes(self) -> int:
        b = C.c_int64(0)
        _check(lib().sbm_coarse_bytes(self._h, C.byref(b)))
        return b.value
