"""ctypes binding of ``libnjf_hip.so`` (C ABI in ``include/njf_hip.h``).

PyTorch is plumbing here: it owns device memory and the stream; every compute call goes through
the C ABI.  There is **no CPU fallback**: if the library is missing or a tensor is not a
contiguous fp32 device tensor the call raises.
"""

from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NJF_HIP_LIB", os.path.join(_HERE, "libnjf_hip.so"))  # override: kernel A/B experiments only

MAX_ACTION_DIM = 10
ZDIM = 384
RESNET_W_FLOATS = 22 * 8192
RESNET_B_FLOATS = 10 * 128 + 32
COLOR_W_FLOATS = 8192
COLOR_B_FLOATS = 96
TRANSFORMER_W_FLOATS = 7 * 8192
TRANSFORMER_B_FLOATS = 3 * 256 + 32
QDIM = 64
JACOBIAN_NONE, JACOBIAN_MLP, JACOBIAN_TRANSFORMER = 0, 1, 2
# MFMA precision of the fused MLPs (include/njf_hip.h: NJF_PRECISION_*).  "f16x2" = fp32 operands split into two
# fp16 (hi+lo), three f16 MFMAs per product block, fp32 accumulation: fp32-class accuracy, ~5x less matrix time.
# "f16f6" = the same hi*hi product, the two 2^-11-sized correction products in block-scaled fp6 (4x the f16 MFMA rate).
# "f16" = PLAIN fp16 products (round 5; BASELINE config 5's "fp16 MFMA fused-MLP"): weights and layer inputs rounded to fp16, fp32
# accumulation, hoisted maps stored in fp16 -- a reduced-precision inference mode with its own stated tolerance (DESIGN.md
# section 5), selectable, never the default.
PRECISIONS = {"f32": 0, "f16x2": 1, "f16f6": 2, "f16": 3}
REDUCED_PRECISIONS = ("f16",)   # modes that are NOT held to the fp32 parity bound
# Default: "f16f6" for the final pass with the proposal networks on "f16x2" (Model.set_precision's policy).  It passes the
# same parity suite as the exact-fp32 path with the same bounds (profiles/r02_parity_margins.json).
DEFAULT_PRECISION = os.environ.get("NJF_PRECISION", "f16f6")
if DEFAULT_PRECISION not in PRECISIONS or DEFAULT_PRECISION in REDUCED_PRECISIONS:
    # the environment may pick among the modes that meet the fp32 parity bound; a reduced mode is chosen per model
    # (Model.set_precision("f16")), by code that knows its tolerance -- never by a variable that every process inherits
    raise ValueError(f"NJF_PRECISION={DEFAULT_PRECISION!r}: the package default must be one of "
                     f"{sorted(set(PRECISIONS) - set(REDUCED_PRECISIONS))}")


def proposal_precision_for(precision: str) -> str:
    """The proposal networks' precision that goes with a decoder precision: the same, except that "f16f6" keeps sample
    PLACEMENT on "f16x2" (an error of 1e-5 in the proposal weights moves samples enough to show up as 3e-4 in depth / flow
    through the positional encoding's 2*pi*512 gain; inside the final pass the same error stays 1e-5).  Re-measured in
    round 2 with the proposal pass forced to "f16f6": depth 3.0e-4 against a bound of 1.0e-4, optical flow 7.8e-4 against
    3.6e-4 (parity cases 1 and 4) for a proposal pass of 3.16 instead of 3.80 ms -- not adopted."""
    return "f16x2" if precision == "f16f6" else precision


def precision_code(precision: Optional[str], jacobian_precision: Optional[str] = None) -> int:
    """include/njf_hip.h: NJF_PRECISION_* (and NJF_PRECISION_MIXED when the Jacobian head runs in another precision)."""
    name = DEFAULT_PRECISION if precision is None else precision
    if name not in PRECISIONS:
        raise ValueError(f"njf_hip: unknown precision {name!r}; choose from {sorted(PRECISIONS)}")
    code = PRECISIONS[name]
    if jacobian_precision is not None and jacobian_precision != name:
        if jacobian_precision not in PRECISIONS:
            raise ValueError(f"njf_hip: unknown precision {jacobian_precision!r}; choose from {sorted(PRECISIONS)}")
        if "f32" in (name, jacobian_precision) or "f16" in (name, jacobian_precision):
            raise ValueError("njf_hip: mixed decoder precisions exist for the two split-precision modes only")
        code |= (PRECISIONS[jacobian_precision] + 1) << 4
    return code

_vp = C.c_void_p


class ResnetFcWeights(C.Structure):
    _fields_ = [
        ("lin_in_w", _vp), ("lin_in_b", _vp),
        ("fc0_w", _vp * 5), ("fc0_b", _vp * 5), ("fc1_w", _vp * 5), ("fc1_b", _vp * 5),
        ("lin_z_w", _vp * 3), ("lin_z_b", _vp * 3),
        ("lin_out_w", _vp), ("lin_out_b", _vp), ("d_out", C.c_int),
    ]


class ColorHeadWeights(C.Structure):
    _fields_ = [("w0", _vp), ("b0", _vp), ("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp)]


class Cameras(C.Structure):
    _fields_ = [
        ("ctxt_w2c", _vp), ("ctxt_k", _vp), ("trgt_w2c", _vp), ("trgt_k", _vp),
        ("z_near", _vp), ("z_far", _vp), ("action", _vp), ("batch", C.c_int), ("action_dim", C.c_int),
    ]


class FeatureMap(C.Structure):
    _fields_ = [("data", _vp), ("height", C.c_int), ("width", C.c_int), ("stride", C.c_int)]


class RenderOutputs(C.Structure):
    _fields_ = [(n, _vp) for n in (
        "rgb", "depth", "step_minmax", "flow", "pos", "pos_warped", "action_features",
        "weights", "density", "color", "sample_flow", "jacobian", "jac_act", "jac_pe", "foot_idx", "foot_w",
        "den_act", "col_in", "col_act", "frame_partials", "trgt_rgb", "trgt_flow", "jac_mask", "den_mask")] + [("dump_f16", C.c_int)]


class PyramidLevel(C.Structure):
    _fields_ = [("feats", _vp), ("channels", C.c_int), ("height", C.c_int), ("width", C.c_int)]


class ActivationDump(C.Structure):
    _fields_ = [("act", _vp), ("pe", _vp), ("foot_idx", _vp), ("foot_w", _vp), ("mask", _vp), ("act_f16", C.c_int)]


class FieldGrid(C.Structure):
    """NjfFieldGrid: node (ix, iy, iz) sits at fmaf(i_c, step[c], origin[c]); linear index (ix*ny + iy)*nz + iz."""
    _fields_ = [("origin", C.c_float * 3), ("step", C.c_float * 3), ("dims", C.c_int * 3)]


_lib = None

_SIGNATURES = {
    "njf_abi_version": ([], C.c_int),
    "njf_rays_per_workgroup": ([], C.c_int),
    "njf_error_string": ([C.c_int], C.c_char_p),
    "njf_pack_resnetfc": ([C.POINTER(ResnetFcWeights), _vp, _vp, _vp, _vp, C.c_int, _vp], C.c_int),
    "njf_pack_resnetfc_ld": ([C.POINTER(ResnetFcWeights), _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp], C.c_int),
    "njf_pack_color_head": ([C.POINTER(ColorHeadWeights), _vp, _vp, C.c_int, _vp], C.c_int),
    "njf_pack_linear": ([_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp], C.c_int),
    "njf_project_features": ([_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp], C.c_int),
    "njf_project_features_ld": ([_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp], C.c_int),
    "njf_project_pyramid": ([C.POINTER(PyramidLevel), C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp],
                            C.c_int),
    "njf_hoisted_channel": ([C.c_int, C.c_int, C.c_int], C.c_int),
    "njf_upsample_concat": ([C.POINTER(PyramidLevel), C.c_int, C.c_int, _vp, _vp], C.c_int),
    "njf_upsample_concat_backward": ([_vp, C.POINTER(PyramidLevel), C.c_int, C.c_int, _vp], C.c_int),
    "njf_solve_action": ([_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _vp, _vp], C.c_int),
    "njf_solve_action_robust": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_float, C.c_float, C.c_int, C.c_float, _vp, _vp], C.c_int),
    "njf_invert_4x4": ([_vp, C.c_int, _vp, _vp], C.c_int),
    "njf_generate_rays": ([_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp], C.c_int),
    "njf_proposal_forward": ([_vp, _vp, C.c_int, C.POINTER(Cameras), C.POINTER(FeatureMap), C.c_int, _vp, _vp,
                              _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_float, _vp, _vp, _vp, C.POINTER(ActivationDump), C.c_int, _vp],
                             C.c_int),
    "njf_render_forward": ([_vp, _vp, C.c_int, C.POINTER(Cameras), C.POINTER(FeatureMap), C.c_int, C.c_int, C.c_int,
                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.POINTER(RenderOutputs), C.c_int, _vp], C.c_int),
    "njf_points_forward": ([_vp, _vp, C.c_int, C.POINTER(Cameras), C.POINTER(FeatureMap), C.c_int, C.c_int, C.c_int,
                            C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp], C.c_int),
    "njf_field_points": ([C.POINTER(FieldGrid), C.c_int, _vp, _vp, C.c_int, _vp, _vp], C.c_int),
    "njf_field_select": ([C.POINTER(FieldGrid), C.POINTER(Cameras), C.c_int, _vp, C.c_float, _vp, _vp, C.c_int, _vp, _vp, C.c_int,
                          _vp, _vp], C.c_int),
    "njf_field_forward": ([C.POINTER(FieldGrid), _vp, _vp, C.c_int, C.POINTER(C.c_float * 3), C.POINTER(Cameras),
                           C.POINTER(FeatureMap), C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                           C.c_int, _vp], C.c_int),
    "njf_field_mesh_vertices": ([C.POINTER(FieldGrid), C.POINTER(Cameras), C.c_int, _vp, _vp, C.c_float, C.c_int, _vp, _vp, _vp, _vp,
                                 _vp, _vp, C.c_int, _vp, _vp, _vp], C.c_int),
    "njf_field_mesh_triangles": ([C.POINTER(FieldGrid), C.c_int, _vp, C.c_float, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp,
                                  _vp], C.c_int),
    "njf_field_forward_at": ([_vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_float * 3), C.POINTER(Cameras),
                              C.POINTER(FeatureMap), C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                              C.c_int, _vp], C.c_int),
    "njf_field_fuse": ([C.POINTER(FieldGrid), C.POINTER(Cameras), C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
                       C.c_int),
    "njf_field_combine": ([_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(Cameras), _vp, _vp, _vp, C.c_int, _vp, _vp, _vp,
                           _vp], C.c_int),
    "njf_field_components": ([C.POINTER(FieldGrid), C.POINTER(Cameras), C.c_int, _vp, C.c_float, _vp, _vp, _vp, C.c_int, _vp,
                              C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "njf_field_band": ([C.POINTER(FieldGrid), C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, C.c_int, _vp,
                        _vp], C.c_int),
    "njf_field_scatter": ([_vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp], C.c_int),
    "njf_field_band_leaks": ([C.POINTER(FieldGrid), C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp], C.c_int),
    "njf_field_twists": ([_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int] + [_vp] * 15 + [C.c_longlong, C.c_int, _vp],
                         C.c_int),
    "njf_field_joints": ([C.POINTER(FieldGrid), C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int,
                          C.c_int, C.c_int, C.c_int] + [_vp] * 9 + [C.c_longlong, C.c_int, _vp], C.c_int),
    "njf_field_pose": ([_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_longlong, C.c_int, _vp], C.c_int),
    "njf_field_commands": ([_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_double, C.c_int, C.c_double] + [_vp] * 11 +
                           [C.c_longlong, C.c_int, _vp], C.c_int),
    "njf_field_commands_metric": ([_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_double, C.c_int,
                                   C.c_double] + [_vp] * 11 + [C.c_longlong, C.c_int, _vp], C.c_int),
    "njf_field_nearest": ([_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(FieldGrid), C.c_double,
                           _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_int, _vp], C.c_int),
    "njf_field_normals": ([_vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(FieldGrid), C.c_double, C.c_int,
                           _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_int, _vp], C.c_int),
    "njf_field_depth_points": ([_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, _vp, _vp,
                                _vp], C.c_int),
    "njf_field_voxels": ([_vp, _vp, C.c_int, C.c_int, C.POINTER(FieldGrid), C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                          C.c_longlong, C.c_int, _vp], C.c_int),
    "njf_field_visible": ([_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                           C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_int, _vp], C.c_int),
    "njf_field_frame": ([_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                         C.c_float, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp], C.c_int),
    "njf_field_tsdf": ([C.POINTER(FieldGrid), _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_float, C.c_float, C.c_float,
                        C.c_float, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "njf_field_tsdf_sample": ([_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(FieldGrid), _vp, _vp, C.c_int, _vp, _vp, _vp, _vp,
                               _vp], C.c_int),
    "njf_pack_resnetfc_backward": ([C.POINTER(ResnetFcWeights), _vp, C.c_int, _vp], C.c_int),
    "njf_resnetfc_backward": ([_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp], C.c_int),
    "njf_pack_transformer_backward": ([_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp], C.c_int),
    "njf_transformer_backward": ([_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp], C.c_int),
    "njf_scatter_footprint": ([_vp, C.c_int, C.c_longlong, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp], C.c_int),
    "njf_bn_act": ([_vp, _vp, _vp, _vp, _vp, C.c_float, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp], C.c_int),
    "njf_relu_backward": ([_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "njf_reduce_frame_partials": ([_vp, C.c_int, _vp, _vp], C.c_int),
    "njf_assemble_frame": ([_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _vp, _vp, _vp], C.c_int),
    "njf_composite_backward": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "njf_alpha_weights": ([_vp, _vp, C.c_int, C.c_int, _vp, _vp], C.c_int),
    "njf_pdf_resample": ([_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_float, C.c_int, _vp, _vp], C.c_int),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library() -> C.CDLL:
    """Load ``libnjf_hip.so`` (built by ``__graft_entry__.build()``); raises if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; "
                "g.build()'`).  There is no CPU fallback for the rendering hot path.")
        lib = C.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib


def _check(code: int) -> None:
    if code == 0:
        return
    msg = load_library().njf_error_string(code).decode()
    if code < 0:
        raise ValueError(f"njf_hip: {msg} (code {code})")
    raise RuntimeError(f"njf_hip: {msg} (hipError_t {code})")


import threading

_call = threading.local()  # per-thread: the device of the tensors handed to the entry point being assembled


def _note_device(t, name: str) -> None:
    """`t`: a tensor, or a Cameras / FeatureMap record (which remembers the device of the tensors it points to)."""
    new = t.device if torch.is_tensor(t) else getattr(t, "_device", None)
    if new is None:
        return
    dev = getattr(_call, "device", None)
    if dev is None:
        _call.device = new
    elif dev != new:
        _call.device = None   # the half-assembled call is abandoned: its device must not leak into the next entry point
        raise ValueError(f"njf_hip: {name} lives on {new} but other arguments of this call live on {dev}; all tensors "
                         "of one call must be on the same GPU")


class _RecordScope:
    """Pointers gathered inside the scope belong to a record built ahead of its call (Cameras, FeatureMap): their device
    is stored on the record instead of leaking into whichever entry point is assembled next."""

    def __enter__(self):
        self.prev = getattr(_call, "device", None)
        _call.device = None
        return self

    def close(self, record):
        record._device = getattr(_call, "device", None)
        return record

    def __exit__(self, *exc):
        _call.device = self.prev
        return False


def device_key(device) -> tuple:
    """Cache key of a device: (type, index) with an index-less ``torch.device('cuda')`` resolved to the CURRENT device -- a
    plain ``str(device)`` would give every GPU of a process the same key."""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        return ("cuda", torch.cuda.current_device())
    return (d.type, d.index)


def cached_device_constant(cache: dict, key: tuple, device, make) -> torch.Tensor:
    """``cache[key]`` (key must end with ``device_key(device)``), built by ``make()`` -- a host tensor -- and uploaded ONCE.  A
    first use inside a HIP-graph capture would be a pageable host-to-device copy inside the capture: refused with a message that
    says what to do (every capture path here warms up with eager steps first, so this only fires on a mis-ordered caller)."""
    t = cache.get(key)
    if t is None:
        d = torch.device(device)
        if d.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("njf: a device constant would be uploaded inside a HIP-graph capture; run one eager step of the same "
                               "shape before capturing (the constant caches are filled on first use)")
        t = make().to(d)
        cache[key] = t
    return t


def map_dtype(precision: Optional[str]) -> torch.dtype:
    """Element type of the hoisted map a network of MFMA ``precision`` reads (include/njf_hip.h: NJF_PRECISION_F16)."""
    return torch.float16 if (DEFAULT_PRECISION if precision is None else precision) == "f16" else torch.float32


def _check_map_dtype(fmap, *precisions: Optional[str]) -> None:
    """The forward kernels read the hoisted map with the element type of their MFMA precision (fp16 maps for "f16", fp32 maps
    otherwise) and the C side cannot tell what an allocation holds: a half map read as fp32 is an out-of-bounds read of twice the
    allocation, an fp32 map read as halves is silent garbage.  Checked here, where the tensor is still known."""
    keep = getattr(fmap, "_keep", None)
    if keep is None:
        return
    for p in precisions:
        if keep.dtype != map_dtype(p):
            raise ValueError(f"njf_hip: the hoisted map is {keep.dtype} but a network of precision "
                             f"{DEFAULT_PRECISION if p is None else p!r} reads {map_dtype(p)} maps (project it with that precision)")


def _ptr(t: Optional[torch.Tensor], name: str = "tensor", dtype: torch.dtype = torch.float32) -> Optional[int]:
    if t is None:
        return None
    problem = None
    if not t.is_cuda:
        problem = f"njf_hip: {name} must live on the GPU (got {t.device}); there is no CPU path"
    elif t.dtype != dtype:
        problem = f"njf_hip: {name} must be {str(dtype).replace('torch.', '')} (got {t.dtype})"
    elif not t.is_contiguous():
        problem = f"njf_hip: {name} must be contiguous"
    if problem is not None:
        _call.device = None   # abandon the half-assembled call (a stale device used to leak into the next one)
        raise ValueError(problem)
    _note_device(t, name)
    return t.data_ptr()


def inverse(m: torch.Tensor) -> torch.Tensor:
    """Batched small-matrix inverse (camera matrices: torch.inverse in rendering/geometry.py:52,64).  fp32 [...,4,4]
    device tensors go through njf_invert_4x4 (one launch); anything else through torch.linalg.inv_ex, which unlike
    torch.linalg.inv does not synchronise with the host for its error check."""
    if m.is_cuda and m.dtype == torch.float32 and m.shape[-2:] == (4, 4) and m.numel() > 0 and not m.requires_grad:
        src = m.contiguous()
        out = torch.empty_like(src)
        _launch("njf_invert_4x4", load_library().njf_invert_4x4, _ptr(src, "matrices"), src.numel() // 16, _ptr(out, "out"))
        return out
    return torch.linalg.inv_ex(m).inverse


def _stream() -> int:
    """The torch stream of the device the call's tensors live on (NOT of the current device: a model loaded on cuda:N
    without torch.cuda.set_device(N) would otherwise launch on device 0's stream with device-N pointers)."""
    dev = getattr(_call, "device", None)
    return torch.cuda.current_stream(dev).cuda_stream


# Optional per-launch timing for bench.py: a list that receives (name, start_event, end_event) for every fused launch,
# recorded on the stream the kernel is launched on.  None (default) = no events, no overhead.
_profile_sink = None


def set_profile_sink(sink) -> None:
    global _profile_sink
    _profile_sink = sink


def _launch(name: str, fn, *args) -> None:
    """Run one C-ABI entry point on the device (and stream) of its tensor arguments, which `_ptr` collected while the
    argument list was built."""
    dev = getattr(_call, "device", None)
    _call.device = None
    if dev is None:
        raise ValueError(f"njf_hip: {name} called without any device tensor")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        if _profile_sink is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _check(fn(*args, stream.cuda_stream))
            e1.record(stream)
            _profile_sink.append((name, e0, e1))
        else:
            _check(fn(*args, stream.cuda_stream))


def make_cameras(ctxt_w2c, ctxt_k, z_near, z_far, trgt_w2c=None, trgt_k=None, action=None, action_dim=None) -> Cameras:
    batch = ctxt_w2c.shape[0]
    a_dim = (0 if action is None else action.shape[-1]) if action_dim is None else action_dim
    with _RecordScope() as scope:
        cams = Cameras(_ptr(ctxt_w2c, "ctxt_w2c"), _ptr(ctxt_k, "ctxt_k"), _ptr(trgt_w2c, "trgt_w2c"),
                       _ptr(trgt_k, "trgt_k"), _ptr(z_near, "z_near"), _ptr(z_far, "z_far"), _ptr(action, "action"),
                       batch, a_dim)
        scope.close(cams)
    cams._keep = (ctxt_w2c, ctxt_k, z_near, z_far, trgt_w2c, trgt_k, action)  # keep tensors alive
    return cams


def make_feature_map(gmap: torch.Tensor) -> FeatureMap:
    """gmap: [B, Hf, Wf, C] channels-last hoisted map (float32; float16 for the networks of the plain-fp16 mode -- the
    precision of the forward call that reads it must agree, which the callers below guarantee by construction)."""
    if gmap.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"njf_hip: gmap must be float32 or float16 (got {gmap.dtype})")
    with _RecordScope() as scope:
        fm = FeatureMap(_ptr(gmap, "gmap", gmap.dtype), gmap.shape[1], gmap.shape[2], gmap.shape[3])
        scope.close(fm)
    fm._keep = gmap
    return fm


# --------------------------------------------------------------------------------------
# packing
# --------------------------------------------------------------------------------------
def pack_resnetfc(params: Dict[str, torch.Tensor], prefix: str, w_out: torch.Tensor, b_out: torch.Tensor,
                  wz: Optional[torch.Tensor] = None, wz_col: int = 0, bz: Optional[torch.Tensor] = None,
                  precision: Optional[str] = None) -> None:
    """``params[prefix + 'lin_in.weight']`` ... (reference ResnetFC names) -> packed blobs.

    ``wz`` [512, ld] / ``bz`` [ld] receive this net's three lin_z layers at columns ``wz_col .. wz_col+383``."""
    def p(name):
        return _ptr(params[prefix + name].detach(), prefix + name)

    src = ResnetFcWeights()
    src.lin_in_w, src.lin_in_b = p("lin_in.weight"), p("lin_in.bias")
    for i in range(5):
        src.fc0_w[i], src.fc0_b[i] = p(f"blocks.{i}.fc_0.weight"), p(f"blocks.{i}.fc_0.bias")
        src.fc1_w[i], src.fc1_b[i] = p(f"blocks.{i}.fc_1.weight"), p(f"blocks.{i}.fc_1.bias")
    for i in range(3):
        src.lin_z_w[i], src.lin_z_b[i] = p(f"lin_z.{i}.weight"), p(f"lin_z.{i}.bias")
    src.lin_out_w, src.lin_out_b = p("lin_out.weight"), p("lin_out.bias")
    src.d_out = params[prefix + "lin_out.weight"].shape[0]
    wz_ptr = bz_ptr = None
    ld = ZDIM
    if wz is not None:
        ld = wz.shape[1]
        if wz.shape[0] != 512 or wz_col + ZDIM > ld or bz is None or bz.numel() != ld:
            raise ValueError("njf_hip: wz must be [512, ld] with wz_col + 384 <= ld and bz [ld]")
        wz_ptr = _ptr(wz, "wz") + 4 * wz_col
        bz_ptr = _ptr(bz, "bz") + 4 * wz_col
    _launch("njf_pack_resnetfc_ld", load_library().njf_pack_resnetfc_ld, C.byref(src), _ptr(w_out), _ptr(b_out), wz_ptr, ld, bz_ptr,
                                               precision_code(precision))


def pack_color_head(params: Dict[str, torch.Tensor], prefix: str, w_out: torch.Tensor, b_out: torch.Tensor,
                    precision: Optional[str] = None) -> None:
    def p(name):
        return _ptr(params[prefix + name].detach(), prefix + name)

    src = ColorHeadWeights(p("0.weight"), p("0.bias"), p("2.weight"), p("2.bias"), p("4.weight"), p("4.bias"))
    _launch("njf_pack_color_head", load_library().njf_pack_color_head, C.byref(src), _ptr(w_out), _ptr(b_out), precision_code(precision))


def pack_linear(weight: torch.Tensor, bias: Optional[torch.Tensor], kind: int, w_out: torch.Tensor,
                b_out: Optional[torch.Tensor] = None, precision: Optional[str] = None) -> None:
    """One Linear [d_out, d_in] -> fragment-major block (see include/njf_hip.h: njf_pack_linear)."""
    d_out, d_in = weight.shape
    _launch("njf_pack_linear", load_library().njf_pack_linear, _ptr(weight.detach().contiguous(), "weight"),
                                          _ptr(None if bias is None else bias.detach().contiguous(), "bias"), d_out, d_in,
                                          kind, _ptr(w_out, "w_out"), _ptr(b_out, "b_out"), precision_code(precision))


def project_features(feats: torch.Tensor, wz: torch.Tensor, bz: torch.Tensor, out: torch.Tensor,
                     precision: Optional[str] = None) -> None:
    """feats [B,512,Hf,Wf]; wz [512,N]; bz [N]; out [B,Hf,Wf,N] (float16 for precision "f16": ``map_dtype``)."""
    b, k, hf, wf = feats.shape
    n = wz.shape[1]
    if k != 512 or wz.shape[0] != 512 or tuple(out.shape) != (b, hf, wf, n):
        raise ValueError("njf_hip: project_features shape mismatch")
    _launch("njf_project_features_ld", load_library().njf_project_features_ld, _ptr(feats), _ptr(wz), n, _ptr(bz), b, hf * wf, n,
            _ptr(out, "out", map_dtype(precision)), precision_code(precision))


def project_pyramid(levels, wz: torch.Tensor, bz: torch.Tensor, out: torch.Tensor, precision: Optional[str] = None) -> None:
    """levels: the encoder's latents [B,C_l,H_l,W_l] in concatenation order (level 0 at the output resolution, channel
    counts summing to 512); wz [512,N]; bz [N]; out [B,H_0,W_0,N] -- the hoisted map of the concatenated, up-sampled
    feature map, without forming it (njf_project_pyramid)."""
    b = levels[0].shape[0]
    n = wz.shape[1]
    if tuple(out.shape) != (b, levels[0].shape[2], levels[0].shape[3], n) or wz.shape[0] != 512:
        raise ValueError("njf_hip: project_pyramid shape mismatch")
    arr = (PyramidLevel * len(levels))()
    keep = []
    ws_floats = 0
    for i, lv in enumerate(levels):
        lv = lv.contiguous()
        keep.append(lv)
        arr[i] = PyramidLevel(_ptr(lv), lv.shape[1], lv.shape[2], lv.shape[3])
        if i > 0 or (map_dtype(precision) == torch.float16 and len(levels) > 1):
            # (plain-fp16 map of a pyramid: the levels are summed in fp32 in the workspace and rounded once)
            ws_floats += b * lv.shape[2] * lv.shape[3] * n
    workspace = torch.empty(max(ws_floats, 1), dtype=torch.float32, device=out.device)
    _launch("njf_project_pyramid", load_library().njf_project_pyramid, arr, len(levels), _ptr(wz), n, _ptr(bz), b, n,
            _ptr(out, "out", map_dtype(precision)), _ptr(workspace), precision_code(precision))


_hoist_order_cache: Dict[tuple, torch.Tensor] = {}


def hoisted_channel_order(block_channels: int, device, precision: str) -> torch.Tensor:
    """pos[f] = position of logical feature f inside a block of ``block_channels`` hoisted-map channels of a network
    packed for MFMA ``precision`` (njf_hoisted_channel: the single definition of that order), as an index tensor on
    ``device``."""
    key = (block_channels, device_key(device), precision)
    if key not in _hoist_order_cache:
        lib = load_library()
        code = PRECISIONS[precision]
        pos = [lib.njf_hoisted_channel(f, block_channels, code) for f in range(block_channels)]
        if min(pos) < 0:
            _check(min(pos))
        _hoist_order_cache[key] = torch.tensor(pos, dtype=torch.long, device=device)
    return _hoist_order_cache[key]


def upsample_concat(levels) -> torch.Tensor:
    """The encoder output cat_l(upsample_l(latent_l)) as a channels-last matrix [B*H_0*W_0, sum C_l] (njf_upsample_concat):
    what the lin_z weight gradients contract against; levels as for project_pyramid."""
    b, _, h0, w0 = levels[0].shape
    arr = (PyramidLevel * len(levels))()
    keep = []
    for i, lv in enumerate(levels):
        lv = lv.contiguous()
        keep.append(lv)
        arr[i] = PyramidLevel(_ptr(lv), lv.shape[1], lv.shape[2], lv.shape[3])
    out = torch.empty(b * h0 * w0, sum(lv.shape[1] for lv in levels), dtype=torch.float32, device=levels[0].device)
    _launch("njf_upsample_concat", load_library().njf_upsample_concat, arr, len(levels), b, _ptr(out))
    return out


def upsample_concat_backward(grad: torch.Tensor, shapes) -> list:
    """Adjoint of ``upsample_concat``: grad [B*H_0*W_0, sum C_l] channels-last -> [gradient of latent l, NCHW] for the
    latents of shapes ``shapes`` = [(B,C_l,H_l,W_l), ...] (njf_upsample_concat_backward)."""
    b, _, h0, w0 = shapes[0]
    n = sum(sh[1] for sh in shapes)
    if tuple(grad.shape) != (b * h0 * w0, n):
        raise ValueError("njf_hip: upsample_concat_backward shape mismatch")
    outs = [torch.empty(tuple(sh), dtype=torch.float32, device=grad.device) for sh in shapes]
    arr = (PyramidLevel * len(shapes))()
    for i, (o, sh) in enumerate(zip(outs, shapes)):
        arr[i] = PyramidLevel(_ptr(o, "latent gradient"), sh[1], sh[2], sh[3])
    _launch("njf_upsample_concat_backward", load_library().njf_upsample_concat_backward, _ptr(grad, "grad"), arr, len(shapes), b)
    return outs


# --------------------------------------------------------------------------------------
# ops
# --------------------------------------------------------------------------------------
def generate_rays(coords, height, width, k_inv, c2w, origins, directions, z) -> None:
    batch, rays = origins.shape[0], origins.shape[1]
    _launch("njf_generate_rays", load_library().njf_generate_rays, _ptr(coords), height, width, _ptr(k_inv), _ptr(c2w), batch, rays,
                                            _ptr(origins), _ptr(directions), _ptr(z))


def _int_ptr(t: torch.Tensor) -> int:
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        _call.device = None
        raise ValueError("njf_hip: foot_idx / mask tensors must be contiguous int32 device tensors")
    _note_device(t, "foot_idx")
    return t.data_ptr()


def proposal_forward(origins, directions, cams: Cameras, fmap: FeatureMap, gmap_offset: int, w_pack, b_pack,
                     bins_in, s_in: int, u, s_out: int, anneal: float, bins_out, weights_out=None,
                     density_out=None, precision: Optional[str] = None,
                     dump: Optional[Dict[str, torch.Tensor]] = None) -> None:
    """``dump`` (training forward): tensors act [11,P,128], pe [P,64], foot_idx [P,4] int32, foot_w [P,4]."""
    rays_per_batch = origins.shape[1]
    dump_ref = None
    if dump is not None:
        if dump["act"].dtype not in (torch.float32, torch.float16):
            raise ValueError(f"njf_hip: activation dumps are float32 or float16 (got {dump['act'].dtype})")
        half = dump["act"].dtype == torch.float16   # 16-bit training storage (training.set_storage_precision)
        dump_ref = C.byref(ActivationDump(_ptr(dump["act"], "act", dump["act"].dtype), _ptr(dump["pe"]), _int_ptr(dump["foot_idx"]),
                                          _ptr(dump["foot_w"]), _int_ptr(dump["mask"]) if dump.get("mask") is not None else None,
                                          int(half)))
    _note_device(cams, "cameras")
    _note_device(fmap, "feature map")
    _check_map_dtype(fmap, precision)
    _launch("njf_proposal_forward", load_library().njf_proposal_forward, 
        _ptr(origins), _ptr(directions), rays_per_batch, C.byref(cams), C.byref(fmap), gmap_offset,
        _ptr(w_pack), _ptr(b_pack), _ptr(bins_in), int(bins_in.dim() > 1), s_in, _ptr(u), int(u.dim() > 1), s_out,
        float(anneal), _ptr(bins_out), _ptr(weights_out), _ptr(density_out), dump_ref, precision_code(precision))


def render_forward(origins, directions, cams: Cameras, fmap: FeatureMap, goff_density: int, goff_jacobian: int,
                   w_all: torch.Tensor, b_density, b_color, b_jacobian, bins, samples: int, outputs: Dict[str, torch.Tensor],
                   jacobian_kind: int = JACOBIAN_MLP, precision: Optional[str] = None,
                   jacobian_precision: Optional[str] = None) -> None:
    """``w_all`` is the single allocation [density | colour | jacobian head] of packed weights; ``jacobian_precision``
    (default: ``precision``) is the MFMA precision the Jacobian head's blob was packed for."""
    rays_per_batch = origins.shape[1]
    out = RenderOutputs()
    dump_f16 = 0
    for name, _ in RenderOutputs._fields_:
        if name == "dump_f16":
            continue
        t = outputs.get(name)
        if name in ("foot_idx", "jac_mask", "den_mask") and t is not None:  # the int32 outputs
            setattr(out, name, _int_ptr(t))
        elif name in ("jac_act", "den_act") and t is not None and t.dtype == torch.float16:   # 16-bit training storage
            setattr(out, name, _ptr(t, name, torch.float16))
            dump_f16 = 1
        else:
            setattr(out, name, _ptr(t, name))
    out.dump_f16 = dump_f16
    base = _ptr(w_all, "w_all")
    w_c = base + 4 * RESNET_W_FLOATS
    with_j = jacobian_kind != JACOBIAN_NONE
    w_j = w_c + 4 * COLOR_W_FLOATS if with_j else None
    _note_device(cams, "cameras")
    _note_device(fmap, "feature map")
    _check_map_dtype(fmap, precision, precision if jacobian_precision is None else jacobian_precision)
    _launch("njf_render_forward", load_library().njf_render_forward, 
        _ptr(origins), _ptr(directions), rays_per_batch, C.byref(cams), C.byref(fmap), goff_density, goff_jacobian,
        jacobian_kind, base, _ptr(b_density), w_c, _ptr(b_color), w_j, _ptr(b_jacobian) if with_j else None,
        _ptr(bins), samples, C.byref(out), precision_code(precision, jacobian_precision))


def points_forward(xyz, dirs, cams: Cameras, fmap: FeatureMap, goff_density: int, goff_jacobian: int, mode: int,
                   w_all, b_density, b_color=None, b_jacobian=None, jacobian_kind: int = JACOBIAN_NONE, density=None,
                   color=None, flow=None, jacobian=None, geo=None, precision: Optional[str] = None,
                   jacobian_precision: Optional[str] = None, features=None) -> None:
    """``features`` [5, B*N, 128] (ABI v18): the ResnetFC head's residual stream after each block (include/njf_hip.h)."""
    points_per_batch = xyz.shape[1]
    if features is not None and tuple(features.shape) != (5, xyz.shape[0] * points_per_batch, 128):
        raise ValueError(f"njf_hip: features must be [5, {xyz.shape[0] * points_per_batch}, 128] (got {tuple(features.shape)})")
    base = _ptr(w_all, "w_all")
    w_c = base + 4 * RESNET_W_FLOATS if mode == 1 else None
    with_j = mode == 1 and jacobian_kind != JACOBIAN_NONE
    w_j = (w_c + 4 * COLOR_W_FLOATS) if with_j else None
    _note_device(cams, "cameras")
    _note_device(fmap, "feature map")
    _check_map_dtype(fmap, precision, precision if jacobian_precision is None else jacobian_precision)
    _launch("njf_points_forward", load_library().njf_points_forward, 
        _ptr(xyz), _ptr(dirs), points_per_batch, C.byref(cams), C.byref(fmap), goff_density, goff_jacobian, mode,
        jacobian_kind if mode == 1 else JACOBIAN_NONE, base, _ptr(b_density), w_c, _ptr(b_color), w_j,
        _ptr(b_jacobian) if with_j else None, _ptr(density), _ptr(color), _ptr(flow), _ptr(jacobian), _ptr(geo),
        _ptr(features, "features"), precision_code(precision, jacobian_precision))


# ---- voxel-grid field extraction (include/njf_hip.h: NjfFieldGrid, njf_field_*) ----------------------------------------
FIELD_SELECT_BLOCK = 1024   # NJF_FIELD_SELECT_BLOCK: list entries one workgroup of njf_field_select covers


def make_field_grid(origin, step, dims) -> FieldGrid:
    return FieldGrid((C.c_float * 3)(*[float(v) for v in origin]), (C.c_float * 3)(*[float(v) for v in step]),
                     (C.c_int * 3)(*[int(v) for v in dims]))


def _int32_ptr(t: Optional[torch.Tensor], name: str) -> Optional[int]:
    return _ptr(t, name, torch.int32)


def field_points(grid: FieldGrid, batch: int, indices, count, capacity: int, xyz: torch.Tensor) -> None:
    """xyz [capacity, 3] <- coordinates of the list's nodes (indices / count: int32 device tensors or None)."""
    if tuple(xyz.shape) != (capacity, 3):
        raise ValueError(f"njf_hip: xyz must be [{capacity}, 3] (got {tuple(xyz.shape)})")
    if indices is not None and indices.numel() < capacity:
        raise ValueError("njf_hip: the index list is shorter than the capacity")
    _launch("njf_field_points", load_library().njf_field_points, C.byref(grid), int(batch), _int32_ptr(indices, "indices"),
            _int32_ptr(count, "count"), int(capacity), _ptr(xyz, "xyz"))


def field_select(grid: FieldGrid, batch: int, capacity: int, out_indices, out_count: torch.Tensor, values=None,
                 threshold: float = 0.0, cams: Optional[Cameras] = None, indices=None, count=None) -> None:
    """Ordered selection (njf_field_select): the entries of the list (indices, count, capacity) with values[i] >= threshold
    and / or inside the context view of ``cams`` -> their global indices in input order into ``out_indices`` (int32, its
    length is the output capacity; None = count only), the true number of survivors into ``out_count`` (int32 [1])."""
    if values is not None and values.numel() < capacity:
        raise ValueError("njf_hip: field_select values are shorter than the capacity")
    if indices is not None and indices.numel() < capacity:
        raise ValueError("njf_hip: the index list is shorter than the capacity")
    if out_count.numel() != 1:
        raise ValueError("njf_hip: out_count must hold one int32")
    blocks = max(1, (capacity + FIELD_SELECT_BLOCK - 1) // FIELD_SELECT_BLOCK)
    workspace = torch.empty(blocks, dtype=torch.int32, device=out_count.device)
    if cams is not None:
        _note_device(cams, "cameras")
    _launch("njf_field_select", load_library().njf_field_select, C.byref(grid), None if cams is None else C.byref(cams),
            int(batch), _ptr(values, "values"), float(threshold), _int32_ptr(indices, "indices"), _int32_ptr(count, "count"),
            int(capacity), _int32_ptr(out_indices, "out_indices"), _int32_ptr(out_count, "out_count"),
            0 if out_indices is None else out_indices.numel(), _int32_ptr(workspace, "workspace"))


def field_forward(grid: FieldGrid, indices, count, capacity: int, cams: Cameras, fmap: FeatureMap, goff_density: int,
                  goff_jacobian: int, mode: int, w_all, b_density, b_color=None, b_jacobian=None,
                  jacobian_kind: int = JACOBIAN_NONE, density=None, color=None, jacobian=None, view_direction=None,
                  precision: Optional[str] = None, jacobian_precision: Optional[str] = None) -> None:
    """``points_forward`` on the nodes of a list (njf_field_forward); outputs are compact [capacity, ...] tensors.  Mode 1
    without ``color`` and without a Jacobian head runs the density network alone."""
    for name, t, width in (("density", density, 1), ("color", color, 3)):
        if t is not None and t.numel() < capacity * width:
            raise ValueError(f"njf_hip: field_forward {name} is shorter than the capacity")
    with_j = mode == 1 and jacobian_kind != JACOBIAN_NONE
    if with_j and (jacobian is None or jacobian.numel() < capacity * 3 * cams.action_dim):
        raise ValueError("njf_hip: field_forward jacobian must be [capacity, 3A]")
    if indices is not None and indices.numel() < capacity:
        raise ValueError("njf_hip: the index list is shorter than the capacity")
    base = _ptr(w_all, "w_all")
    with_c = mode == 1 and (color is not None or with_j)
    w_c = base + 4 * RESNET_W_FLOATS if with_c else None
    w_j = (w_c + 4 * COLOR_W_FLOATS) if with_j else None
    direction = None if view_direction is None else C.byref((C.c_float * 3)(*[float(v) for v in view_direction]))
    _note_device(cams, "cameras")
    _note_device(fmap, "feature map")
    _check_map_dtype(fmap, precision, *([precision if jacobian_precision is None else jacobian_precision] if with_j else []))
    _launch("njf_field_forward", load_library().njf_field_forward, C.byref(grid), _int32_ptr(indices, "indices"),
            _int32_ptr(count, "count"), int(capacity), direction, C.byref(cams), C.byref(fmap), goff_density, goff_jacobian,
            mode, jacobian_kind if mode == 1 else JACOBIAN_NONE, base, _ptr(b_density), w_c,
            _ptr(b_color) if with_c else None, w_j, _ptr(b_jacobian) if with_j else None, _ptr(density, "density"),
            _ptr(color, "color"), _ptr(jacobian, "jacobian") if with_j else None,
            precision_code(precision, jacobian_precision if with_j else None))


# ---- isosurface mesh of a scalar on the grid (include/njf_hip.h: njf_field_mesh_*, njf_field_forward_at) ----------------
FIELD_MESH_BLOCK = 1024     # NJF_FIELD_MESH_BLOCK: nodes (cells) one workgroup of the meshing launches covers
FIELD_MESH_COUNT = 1        # NJF_FIELD_MESH_COUNT: the counting launch and the scan
FIELD_MESH_EMIT = 2         # NJF_FIELD_MESH_EMIT: the emitting launch of a count made before


def field_mesh_workspace(total_nodes: int, device) -> torch.Tensor:
    return torch.empty(max(1, (total_nodes + FIELD_MESH_BLOCK - 1) // FIELD_MESH_BLOCK), dtype=torch.int32, device=device)


def _byte_ptr(t: Optional[torch.Tensor], name: str) -> Optional[int]:
    if t is not None and t.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"njf_hip: {name} must be uint8 or bool (got {t.dtype})")
    return None if t is None else _ptr(t.view(torch.uint8), name, torch.uint8)


def field_mesh_vertices(grid: FieldGrid, batch: int, values: torch.Tensor, threshold: float, phase: int, edge_mask: torch.Tensor,
                        vertex_offset: torch.Tensor, vertex_count: torch.Tensor, workspace: torch.Tensor, valid=None,
                        cams: Optional[Cameras] = None, vertex_node=None, vertex_edge=None, vertex_t=None, vertices=None) -> None:
    """njf_field_mesh_vertices: edge masks, per-node vertex offsets, the true vertex count and -- with FIELD_MESH_EMIT -- the
    rows of the first ``vertex_node.numel()`` vertices.  ``values`` fp32 [B*N]; ``valid`` uint8 / bool [B*N] or None; ``cams``:
    the frustum predicate of ``field_select`` joins ``valid``."""
    total = batch * grid.dims[0] * grid.dims[1] * grid.dims[2]
    for name, t in (("values", values), ("edge_mask", edge_mask), ("vertex_offset", vertex_offset)) + (
            (("valid", valid),) if valid is not None else ()):
        if t.numel() != total:
            raise ValueError(f"njf_hip: field_mesh_vertices {name} must hold batch * nx*ny*nz = {total} elements")
    if vertex_count.numel() != 1 or workspace.numel() < (total + FIELD_MESH_BLOCK - 1) // FIELD_MESH_BLOCK:
        raise ValueError("njf_hip: field_mesh_vertices needs one int32 count and a workspace of ceil(B*N / FIELD_MESH_BLOCK)")
    capacity = 0 if vertex_node is None else vertex_node.numel()
    if capacity and (vertex_edge.numel() != capacity or vertex_t.numel() != capacity or vertices.numel() != 3 * capacity):
        raise ValueError("njf_hip: field_mesh_vertices outputs must share one capacity")
    if cams is not None:
        _note_device(cams, "cameras")
    _launch("njf_field_mesh_vertices", load_library().njf_field_mesh_vertices, C.byref(grid),
            None if cams is None else C.byref(cams), int(batch), _ptr(values, "values"), _byte_ptr(valid, "valid"),
            float(threshold), int(phase), _byte_ptr(edge_mask, "edge_mask"), _int32_ptr(vertex_offset, "vertex_offset"),
            _int32_ptr(vertex_node, "vertex_node"), _byte_ptr(vertex_edge, "vertex_edge"), _ptr(vertex_t, "vertex_t"),
            _ptr(vertices, "vertices"), capacity, _int32_ptr(vertex_count, "vertex_count"), _int32_ptr(workspace, "workspace"))


def field_mesh_triangles(grid: FieldGrid, batch: int, values: torch.Tensor, threshold: float, phase: int,
                         edge_mask: torch.Tensor, vertex_offset: torch.Tensor, triangle_count: torch.Tensor,
                         workspace: torch.Tensor, triangles=None, triangle_cell=None) -> None:
    """njf_field_mesh_triangles on the masks and offsets ``field_mesh_vertices`` wrote: the true triangle count and -- with
    FIELD_MESH_EMIT -- the first ``triangle_cell.numel()`` triangles (vertex ranks) with their global cell index."""
    total = batch * grid.dims[0] * grid.dims[1] * grid.dims[2]
    if values.numel() != total or edge_mask.numel() != total or vertex_offset.numel() != total:
        raise ValueError(f"njf_hip: field_mesh_triangles per-node arrays must hold batch * nx*ny*nz = {total} elements")
    if triangle_count.numel() != 1 or workspace.numel() < (total + FIELD_MESH_BLOCK - 1) // FIELD_MESH_BLOCK:
        raise ValueError("njf_hip: field_mesh_triangles needs one int32 count and a workspace of ceil(B*N / FIELD_MESH_BLOCK)")
    capacity = 0 if triangle_cell is None else triangle_cell.numel()
    if capacity and triangles.numel() != 3 * capacity:
        raise ValueError("njf_hip: field_mesh_triangles triangles must be [capacity, 3]")
    _launch("njf_field_mesh_triangles", load_library().njf_field_mesh_triangles, C.byref(grid), int(batch),
            _ptr(values, "values"), float(threshold), int(phase), _byte_ptr(edge_mask, "edge_mask"),
            _int32_ptr(vertex_offset, "vertex_offset"), _int32_ptr(triangles, "triangles"),
            _int32_ptr(triangle_cell, "triangle_cell"), capacity, _int32_ptr(triangle_count, "triangle_count"),
            _int32_ptr(workspace, "workspace"))


def field_forward_at(xyz: torch.Tensor, node: torch.Tensor, count, capacity: int, nodes_per_batch: int, cams: Cameras,
                     fmap: FeatureMap, goff_density: int, goff_jacobian: int, w_all, b_density, b_color, b_jacobian=None,
                     jacobian_kind: int = JACOBIAN_NONE, density=None, color=None, jacobian=None, view_direction=None,
                     precision: Optional[str] = None, jacobian_precision: Optional[str] = None) -> None:
    """The decoder at stored positions of a ragged batch (njf_field_forward_at): row i is the point ``xyz[i]`` of batch element
    ``node[i] // nodes_per_batch``; outputs are [capacity, ...] tensors, rows past the device count are left untouched."""
    if xyz.numel() < 3 * capacity or node.numel() < capacity:
        raise ValueError("njf_hip: field_forward_at xyz / node are shorter than the capacity")
    for name, t, width in (("density", density, 1), ("color", color, 3)):
        if t is not None and t.numel() < capacity * width:
            raise ValueError(f"njf_hip: field_forward_at {name} is shorter than the capacity")
    with_j = jacobian_kind != JACOBIAN_NONE
    if with_j and (jacobian is None or jacobian.numel() < capacity * 3 * cams.action_dim):
        raise ValueError("njf_hip: field_forward_at jacobian must be [capacity, 3A]")
    base = _ptr(w_all, "w_all")
    w_c = base + 4 * RESNET_W_FLOATS
    w_j = (w_c + 4 * COLOR_W_FLOATS) if with_j else None
    direction = None if view_direction is None else C.byref((C.c_float * 3)(*[float(v) for v in view_direction]))
    _note_device(cams, "cameras")
    _note_device(fmap, "feature map")
    _check_map_dtype(fmap, precision, *([precision if jacobian_precision is None else jacobian_precision] if with_j else []))
    _launch("njf_field_forward_at", load_library().njf_field_forward_at, _ptr(xyz, "xyz"), _int32_ptr(node, "node"),
            _int32_ptr(count, "count"), int(capacity), int(nodes_per_batch), direction, C.byref(cams), C.byref(fmap),
            goff_density, goff_jacobian, jacobian_kind, base, _ptr(b_density), w_c, _ptr(b_color), w_j,
            _ptr(b_jacobian) if with_j else None, _ptr(density, "density"), _ptr(color, "color"),
            _ptr(jacobian, "jacobian") if with_j else None, precision_code(precision, jacobian_precision if with_j else None))


# ---- fusion of several context views (include/njf_hip.h: njf_field_fuse, njf_field_combine) ----------------------------
FIELD_MAX_VIEWS = 8         # NJF_FIELD_MAX_VIEWS: views per scene
FIELD_FUSE_MEAN = 0         # NJF_FIELD_FUSE_MEAN: mean of the views that see the node
FIELD_FUSE_MIN = 1          # NJF_FIELD_FUSE_MIN: carving -- occupied only if every view that sees the node says so
FIELD_FUSE_MAX = 2          # NJF_FIELD_FUSE_MAX
FIELD_FUSE_MODES = {"mean": FIELD_FUSE_MEAN, "min": FIELD_FUSE_MIN, "max": FIELD_FUSE_MAX}


def field_fuse(grid: FieldGrid, scenes: int, views: int, values: torch.Tensor, mode: int, min_views: int, fused: torch.Tensor,
               seen=None, valid=None, cams: Optional[Cameras] = None) -> None:
    """njf_field_fuse: per-view ``values`` fp32 [G*V*N] -> ``fused`` fp32 [G*N], ``seen`` (uint8 bitmask of the views whose
    frustum holds the node) and ``valid`` (uint8 / bool: at least ``min_views`` of them) [G*N]; ``cams`` None: every view sees
    every node."""
    nodes = grid.dims[0] * grid.dims[1] * grid.dims[2]
    if values.numel() != scenes * views * nodes:
        raise ValueError(f"njf_hip: field_fuse values must hold scenes * views * nx*ny*nz = {scenes * views * nodes} elements")
    for name, t in (("fused", fused), ("seen", seen), ("valid", valid)):
        if t is not None and t.numel() != scenes * nodes:
            raise ValueError(f"njf_hip: field_fuse {name} must hold scenes * nx*ny*nz = {scenes * nodes} elements")
    if cams is not None:
        _note_device(cams, "cameras")
    _launch("njf_field_fuse", load_library().njf_field_fuse, C.byref(grid), None if cams is None else C.byref(cams), int(scenes),
            int(views), _ptr(values, "values"), int(mode), int(min_views), _ptr(fused, "fused"), _byte_ptr(seen, "seen"),
            _byte_ptr(valid, "valid"))


def field_combine(xyz: torch.Tensor, node: torch.Tensor, count, capacity: int, nodes_per_scene: int, views: int,
                  cams: Optional[Cameras], density, color=None, jacobian=None, action_dim: int = 0, out_color=None,
                  out_jacobian=None, out_views=None) -> None:
    """njf_field_combine: the density-weighted combination of the per-view rows (entry-major, row ``i*views + v``) at the
    positions ``xyz`` [capacity, 3] of the scenes ``node // nodes_per_scene`` -> ``out_color`` [capacity, 3], ``out_jacobian``
    [capacity, 3A] and ``out_views`` (uint8 [capacity]: the views whose frustum holds the position; all of them without
    ``cams``).  Rows past the device count are left untouched."""
    if xyz.numel() < 3 * capacity or node.numel() < capacity:
        raise ValueError("njf_hip: field_combine xyz / node are shorter than the capacity")
    for name, t, width in (("density", density, views), ("color", color, 3 * views), ("jacobian", jacobian, 3 * action_dim * views),
                           ("out_color", out_color, 3), ("out_jacobian", out_jacobian, 3 * action_dim), ("out_views", out_views, 1)):
        if t is not None and t.numel() < capacity * width:
            raise ValueError(f"njf_hip: field_combine {name} is shorter than the capacity")
    if cams is not None:
        _note_device(cams, "cameras")
    _launch("njf_field_combine", load_library().njf_field_combine, _ptr(xyz, "xyz"), _int32_ptr(node, "node"),
            _int32_ptr(count, "count"), int(capacity), int(nodes_per_scene), int(views), None if cams is None else C.byref(cams),
            _ptr(density, "density"), _ptr(color, "color"), _ptr(jacobian, "jacobian"), int(action_dim), _ptr(out_color, "out_color"),
            _ptr(out_jacobian, "out_jacobian"), _byte_ptr(out_views, "out_views"))


# ---- connected components of the inside nodes (include/njf_hip.h: njf_field_components) ---------------------------------
FIELD_COMPONENTS_BLOCK = 1024          # NJF_FIELD_COMPONENTS_BLOCK: nodes one workgroup of the four launches covers
FIELD_COMPONENTS_CONNECTIVITIES = (6, 14)
FIELD_COMPONENTS_PHASES = (1, 2, 4, 8)  # NJF_FIELD_COMPONENTS_INIT / _MERGE / _LABEL / _SIZES: one launch each
FIELD_COMPONENTS_ALL = 15              # NJF_FIELD_COMPONENTS_ALL
FIELD_COMPONENTS_E_LOCAL = 1           # NJF_FIELD_COMPONENTS_E_*: bits of the status word (an iteration cap was passed)
FIELD_COMPONENTS_E_FIND = 2
FIELD_COMPONENTS_E_UNION = 4


def field_components(grid: FieldGrid, batch: int, connectivity: int, labels: torch.Tensor, sizes: torch.Tensor,
                     count: torch.Tensor, status: torch.Tensor, values=None, threshold: float = 0.0, valid=None,
                     cams: Optional[Cameras] = None, indices=None, list_count=None, capacity: int = 0, keys=None,
                     phase: int = FIELD_COMPONENTS_ALL, workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_components: ``labels`` / ``sizes`` (int32 [B*N]), ``count`` and ``status`` (int32 [1]) of the components of the
    inside nodes -- dense form: ``values`` >= ``threshold`` with ``valid`` and the frustum of ``cams``; list form: the first
    min(``list_count``, ``capacity``) entries of the ascending ``indices``.  ``keys``: int32 [B*N] (dense) or [capacity]
    (list), joining only nodes of equal key.  ``phase`` / ``workspace`` (int32 [2*B*N], [3*B*N] for a keyed list): run the
    four launches one by one on a workspace of the caller's, to time them apart."""
    total = batch * grid.dims[0] * grid.dims[1] * grid.dims[2]
    for name, t in (("labels", labels), ("sizes", sizes), ("values", values), ("valid", valid)):
        if t is not None and t.numel() != total:
            raise ValueError(f"njf_hip: field_components {name} must hold batch * nx*ny*nz = {total} elements")
    if count.numel() != 1 or status.numel() != 1:
        raise ValueError("njf_hip: field_components needs one int32 count and one int32 status")
    if indices is not None and indices.numel() < capacity:
        raise ValueError("njf_hip: the index list is shorter than the capacity")
    if keys is not None and keys.numel() < (total if indices is None else capacity):
        raise ValueError("njf_hip: field_components keys are shorter than the nodes (dense form) / the capacity (list form)")
    slabs = 3 if (indices is not None and keys is not None) else 2
    if workspace is None:
        workspace = torch.empty(slabs * max(total, 1), dtype=torch.int32, device=labels.device)
    elif workspace.numel() < slabs * total:
        raise ValueError(f"njf_hip: field_components workspace must hold {slabs} * batch * nx*ny*nz int32")
    if cams is not None:
        _note_device(cams, "cameras")
    _launch("njf_field_components", load_library().njf_field_components, C.byref(grid), None if cams is None else C.byref(cams),
            int(batch), _ptr(values, "values"), float(threshold), _byte_ptr(valid, "valid"), _int32_ptr(indices, "indices"),
            _int32_ptr(list_count, "count"), int(capacity), _int32_ptr(keys, "keys"), int(connectivity), int(phase),
            _int32_ptr(labels, "labels"), _int32_ptr(sizes, "sizes"), _int32_ptr(count, "component_count"),
            _int32_ptr(status, "status"), _int32_ptr(workspace, "workspace"))


# ---- coarse-to-fine band (include/njf_hip.h: njf_field_band, njf_field_scatter, njf_field_band_leaks) --------------------
FIELD_BAND_BLOCK = 1024                # NJF_FIELD_BAND_BLOCK: nodes one workgroup of the band launches covers
FIELD_BAND_FACTORS = (2, 4, 8, 16)
FIELD_BAND_MAX_DILATE = 2


def field_band_blocks(dims, factor: int):
    """Blocks per axis ``m_c = (n_c - 1) / factor`` of a fine grid; ValueError unless the factor is 2, 4, 8 or 16 and every axis
    has ``(n_c - 1) % factor == 0`` and ``n_c >= factor + 1``."""
    if isinstance(factor, bool) or not isinstance(factor, int) or factor not in FIELD_BAND_FACTORS:
        raise ValueError(f"njf_hip: the coarse factor must be one of {FIELD_BAND_FACTORS} (got {factor!r})")
    dims = tuple(int(d) for d in dims)
    if any(d < factor + 1 or (d - 1) % factor for d in dims):
        raise ValueError(f"njf_hip: coarse = {factor} needs (n - 1) % {factor} == 0 and n >= {factor + 1} on every axis of the "
                         f"grid (got dims {dims})")
    return tuple((d - 1) // factor for d in dims)


def field_band(grid: FieldGrid, factor: int, dilate: int, batch: int, coarse_values: torch.Tensor, coarse_threshold: float,
               block_active: torch.Tensor, band: torch.Tensor, out_indices, out_count: torch.Tensor, coarse_valid=None) -> None:
    """njf_field_band: coarse values fp32 [B*M] (and ``coarse_valid`` uint8 / bool [B*M]) -> ``block_active`` (uint8 [B*Nb]),
    ``band`` (uint8 [B*N]), the ascending global indices of the band nodes into ``out_indices`` (int32, its length is the
    capacity; None = count only) and their true number into ``out_count`` (int32 [1])."""
    m = field_band_blocks(tuple(grid.dims), factor)
    if isinstance(dilate, bool) or not isinstance(dilate, int) or not 0 <= dilate <= FIELD_BAND_MAX_DILATE:
        raise ValueError(f"njf_hip: the band dilation must be 0, 1 or 2 (got {dilate!r})")
    if not math.isfinite(float(coarse_threshold)):
        raise ValueError("njf_hip: the coarse threshold must be finite")
    nodes = grid.dims[0] * grid.dims[1] * grid.dims[2]
    coarse_nodes, blocks = (m[0] + 1) * (m[1] + 1) * (m[2] + 1), m[0] * m[1] * m[2]
    for name, t, size in (("coarse_values", coarse_values, batch * coarse_nodes), ("coarse_valid", coarse_valid, batch * coarse_nodes),
                          ("block_active", block_active, batch * blocks), ("band", band, batch * nodes)):
        if t is not None and t.numel() != size:
            raise ValueError(f"njf_hip: field_band {name} must hold {size} elements (got {t.numel()})")
    if out_count.numel() != 1:
        raise ValueError("njf_hip: out_count must hold one int32")
    workspace = torch.empty(max(1, (batch * nodes + FIELD_BAND_BLOCK - 1) // FIELD_BAND_BLOCK), dtype=torch.int32,
                            device=out_count.device)
    _launch("njf_field_band", load_library().njf_field_band, C.byref(grid), int(factor), int(dilate), int(batch),
            _ptr(coarse_values, "coarse_values"), _byte_ptr(coarse_valid, "coarse_valid"), float(coarse_threshold),
            _byte_ptr(block_active, "block_active"), _byte_ptr(band, "band"), _int32_ptr(out_indices, "out_indices"),
            _int32_ptr(out_count, "out_count"), 0 if out_indices is None else out_indices.numel(),
            _int32_ptr(workspace, "workspace"))


def field_scatter(values: torch.Tensor, indices: torch.Tensor, count, capacity: int, out: torch.Tensor) -> None:
    """njf_field_scatter: ``out.reshape(-1)[indices[i]] = values[i]`` for the first min(``count``, ``capacity``) rows (``count``:
    int32 device tensor or None); indices outside ``out`` are skipped, rows past the count never read."""
    if values.numel() < capacity or indices.numel() < capacity:
        raise ValueError("njf_hip: field_scatter values / indices are shorter than the capacity")
    if out.numel() >= 2 ** 31:
        raise ValueError("njf_hip: field_scatter out must stay below 2**31 elements")
    _launch("njf_field_scatter", load_library().njf_field_scatter, _ptr(values, "values"), _int32_ptr(indices, "indices"),
            _int32_ptr(count, "count"), int(capacity), _ptr(out, "out"), out.numel())


def field_band_leaks(grid: FieldGrid, batch: int, band: torch.Tensor, indices: torch.Tensor, count, capacity: int,
                     leaks: torch.Tensor) -> None:
    """njf_field_band_leaks: ``leaks`` (int32 [1]) <- the number of the list's inside nodes (ascending ``indices``, the first
    min(``count``, ``capacity``)) with a neighbour along one of the seven mesh directions, either sign, outside the band."""
    if band.numel() != batch * grid.dims[0] * grid.dims[1] * grid.dims[2]:
        raise ValueError("njf_hip: field_band_leaks band must hold batch * nx*ny*nz bytes")
    if indices.numel() < capacity:
        raise ValueError("njf_hip: the index list is shorter than the capacity")
    if leaks.numel() != 1:
        raise ValueError("njf_hip: leaks must hold one int32")
    _launch("njf_field_band_leaks", load_library().njf_field_band_leaks, C.byref(grid), int(batch), _byte_ptr(band, "band"),
            _int32_ptr(indices, "indices"), _int32_ptr(count, "count"), int(capacity), _int32_ptr(leaks, "leaks"))


# ---- rigid twists per part and command channel (include/njf_hip.h: njf_field_twists) -------------------------------------
FIELD_TWISTS_CHUNK = 4096              # NJF_FIELD_TWISTS_CHUNK: consecutive rows one workgroup scans for one part
FIELD_TWISTS_MAX_PARTS = 256           # NJF_FIELD_TWISTS_MAX_PARTS
FIELD_TWISTS_EMPTY = 1                 # NJF_FIELD_TWISTS_EMPTY: status bit, no row of positive weight
FIELD_TWISTS_TRANSLATION = 2           # NJF_FIELD_TWISTS_TRANSLATION: status bit, omega is not determined (set to 0)
FIELD_TWISTS_PHASES = (1, 2, 4, 8, 16, 32, 64)   # NJF_FIELD_TWISTS_CLEAR .. _RESIDUAL_SUM: the memset and one launch each
FIELD_TWISTS_PHASE_NAMES = ("clear", "sums", "centroid", "moments", "solve", "residual", "residual_sum")
FIELD_TWISTS_ALL = 127                 # NJF_FIELD_TWISTS_ALL


def field_twists_workspace(rows: int, parts: int, action_dim: int) -> int:
    """Doubles of workspace njf_field_twists needs: NJF_FIELD_TWISTS_STRIDE(A) * K * ceil(n / NJF_FIELD_TWISTS_CHUNK)."""
    return (6 + 7 * action_dim) * parts * ((rows + FIELD_TWISTS_CHUNK - 1) // FIELD_TWISTS_CHUNK)


def _double_ptr(t: Optional[torch.Tensor], name: str) -> Optional[int]:
    return _ptr(t, name, torch.float64)


def field_twists(xyz: torch.Tensor, jacobian: torch.Tensor, labels: torch.Tensor, parts: torch.Tensor, out: dict,
                 weights=None, count=None, parts_count=None, phase: int = FIELD_TWISTS_ALL,
                 workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_twists on ``xyz`` [n, 3], ``jacobian`` [n, A, 3] (fp32), ``labels`` [n] and ``parts`` [K] (int32): ``out`` maps
    the names of the C outputs -- labels, count, nodes, status (int32), weight, centroid, omega, velocity, energy, residual, q,
    p, l (float64), row_residual (fp32) -- to tensors of their shapes.  ``phase`` / ``workspace`` (float64,
    ``field_twists_workspace`` elements): run the launches one by one on a workspace of the caller's, to time them apart."""
    n, k = xyz.shape[0], parts.numel()
    if jacobian.dim() != 3 or jacobian.shape[0] != n or jacobian.shape[2] != 3 or tuple(xyz.shape) != (n, 3):
        raise ValueError("njf_hip: field_twists needs xyz [n, 3] and jacobian [n, A, 3]")
    a = jacobian.shape[1]
    if labels.numel() != n or (weights is not None and weights.numel() != n):
        raise ValueError("njf_hip: field_twists labels / weights must hold one entry per row")
    for name, t in (("count", count), ("parts_count", parts_count), ("out count", out["count"])):
        if t is not None and t.numel() != 1:
            raise ValueError(f"njf_hip: field_twists {name} must hold one int32")
    sizes = dict(labels=k, nodes=k, status=k, weight=k, centroid=3 * k, omega=3 * a * k, velocity=3 * a * k, energy=a * k,
                 residual=a * k, q=6 * k, p=3 * a * k, l=3 * a * k, row_residual=n)
    for name, size in sizes.items():
        if out[name].numel() != size:
            raise ValueError(f"njf_hip: field_twists output {name} must hold {size} elements (got {out[name].numel()})")
    need = field_twists_workspace(n, k, a)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.float64, device=xyz.device)
    _launch("njf_field_twists", load_library().njf_field_twists, _ptr(xyz, "xyz"), _ptr(jacobian, "jacobian"),
            _int32_ptr(labels, "labels"), _ptr(weights, "weights"), _int32_ptr(count, "count"), int(n), int(a),
            _int32_ptr(parts, "parts"), _int32_ptr(parts_count, "parts_count"), int(k), _int32_ptr(out["labels"], "out labels"),
            _int32_ptr(out["count"], "out count"), _int32_ptr(out["nodes"], "nodes"), _int32_ptr(out["status"], "status"),
            *[_double_ptr(out[f], f) for f in ("weight", "centroid", "omega", "velocity", "energy", "residual", "q", "p", "l")],
            _ptr(out["row_residual"], "row_residual"), _double_ptr(workspace, "workspace"), int(workspace.numel()), int(phase))


# ---- joints between parts: grid contacts and relative twists (include/njf_hip.h: njf_field_joints) ------------------------
FIELD_JOINTS_MAX = 4096                # NJF_FIELD_JOINTS_MAX: rows of the joint list
FIELD_JOINTS_PHASES = (1, 2, 4, 8, 16)  # NJF_FIELD_JOINTS_CLEAR .. _TWISTS: the two memsets and one launch each
FIELD_JOINTS_PHASE_NAMES = ("clear", "slots", "contacts", "list", "twists")
FIELD_JOINTS_ALL = 31                  # NJF_FIELD_JOINTS_ALL
FIELD_JOINTS_PER_LANE = 32             # NJF_FIELD_JOINTS_PER_LANE: the contacts launch without the in-wave combination


def field_joints_workspace(total_nodes: int, parts: int) -> int:
    """64-bit words of workspace njf_field_joints needs: NJF_FIELD_JOINTS_WORKSPACE(B*N, K) -- the K x K x 4 pair table and the
    int32 slot volume of B*N nodes."""
    return 4 * parts * parts + (total_nodes + 1) // 2


def field_joints(grid: FieldGrid, batch: int, indices: torch.Tensor, labels: torch.Tensor, parts: torch.Tensor,
                 part_status: torch.Tensor, centroid: torch.Tensor, omega: torch.Tensor, velocity: torch.Tensor, out: dict,
                 count=None, parts_count=None, connectivity: int = 6, min_contacts: int = 1, phase: int = FIELD_JOINTS_ALL,
                 workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_joints on the list ``indices`` / ``labels`` [n] (int32) of a cloud on ``grid`` x ``batch`` and the part list and
    twists ``parts``, ``part_status`` [K] (int32), ``centroid`` [K, 3], ``omega``, ``velocity`` [K, A, 3] (float64): ``out`` maps
    the names of the C outputs -- part_a, part_b, status [J], count [1] (int32), contacts [J] (int64), anchor [J, 3], omega,
    velocity [J, A, 3] (float64) -- to tensors of their shapes.  ``phase`` / ``workspace`` (int64, ``field_joints_workspace``
    elements): run the launches one by one on a workspace of the caller's, to time them apart."""
    n, k, j = indices.numel(), parts.numel(), out["part_a"].numel()
    if omega.dim() != 3 or omega.shape[0] != k or omega.shape[2] != 3 or velocity.shape != omega.shape:
        raise ValueError("njf_hip: field_joints needs omega and velocity [K, A, 3]")
    a = omega.shape[1]
    if labels.numel() != n or part_status.numel() != k or centroid.numel() != 3 * k:
        raise ValueError("njf_hip: field_joints needs one label per row, one status and one centroid per part")
    for name, t in (("count", count), ("parts_count", parts_count), ("out count", out["count"])):
        if t is not None and t.numel() != 1:
            raise ValueError(f"njf_hip: field_joints {name} must hold one int32")
    sizes = dict(part_a=j, part_b=j, status=j, contacts=j, anchor=3 * j, omega=3 * a * j, velocity=3 * a * j)
    for name, size in sizes.items():
        if out[name].numel() != size:
            raise ValueError(f"njf_hip: field_joints output {name} must hold {size} elements (got {out[name].numel()})")
    total = int(batch) * grid.dims[0] * grid.dims[1] * grid.dims[2]
    if workspace is None:
        workspace = torch.empty(field_joints_workspace(total, k), dtype=torch.int64, device=indices.device)
    _launch("njf_field_joints", load_library().njf_field_joints, C.byref(grid), int(batch), _int32_ptr(indices, "indices"),
            _int32_ptr(labels, "labels"), _int32_ptr(count, "count"), int(n), _int32_ptr(parts, "parts"),
            _int32_ptr(parts_count, "parts_count"), int(k), _int32_ptr(part_status, "part_status"),
            _double_ptr(centroid, "centroid"), _double_ptr(omega, "omega"), _double_ptr(velocity, "velocity"), int(a),
            int(connectivity), int(min_contacts), int(j), _int32_ptr(out["part_a"], "part_a"), _int32_ptr(out["part_b"], "part_b"),
            _ptr(out["contacts"], "contacts", torch.int64), _int32_ptr(out["status"], "status"),
            _int32_ptr(out["count"], "out count"), _double_ptr(out["anchor"], "anchor"), _double_ptr(out["omega"], "out omega"),
            _double_ptr(out["velocity"], "out velocity"), _ptr(workspace, "workspace", torch.int64), int(workspace.numel()),
            int(phase))


# ---- posing the parts under a command: twist exponentials along the tree (include/njf_hip.h: njf_field_pose) ---------------
FIELD_POSE_MAX_COMMANDS = 65535        # NJF_FIELD_POSE_MAX_COMMANDS
FIELD_POSE_LINKS, FIELD_POSE_CHAIN, FIELD_POSE_POINTS = 1, 2, 4   # NJF_FIELD_POSE_LINKS, _CHAIN, _POINTS: one launch each
FIELD_POSE_PHASES = (FIELD_POSE_LINKS, FIELD_POSE_CHAIN, FIELD_POSE_POINTS)
FIELD_POSE_PHASE_NAMES = ("links", "chain", "points")
FIELD_POSE_ALL = 7                     # NJF_FIELD_POSE_ALL
FIELD_POSE_STAGED = 8                  # NJF_FIELD_POSE_STAGED: the points launch with one command's transforms staged in LDS
FIELD_POSE_WIDE = 16                   # NJF_FIELD_POSE_WIDE: the points launch with 16-byte stores through an LDS tile


def field_pose_workspace(commands: int, parts: int) -> int:
    """Doubles of workspace njf_field_pose needs: NJF_FIELD_POSE_WORKSPACE(M, K) -- the link motions [M, K, 12] and the int32
    link bits of the K slots."""
    return 12 * commands * parts + (parts + 1) // 2


def field_pose(parts: torch.Tensor, part_status: torch.Tensor, centroid: torch.Tensor, omega: torch.Tensor,
               velocity: torch.Tensor, commands: torch.Tensor, out: dict, parts_count=None, joints: Optional[dict] = None,
               points: Optional[dict] = None, phase: int = FIELD_POSE_ALL, workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_pose on the part list and twists ``parts``, ``part_status`` [K] (int32), ``centroid`` [K, 3], ``omega``,
    ``velocity`` [K, A, 3] (float64) and ``commands`` [M, A] (fp32).  ``out`` maps rotation [M, K, 3, 3], translation [M, K, 3]
    (float64), status and depth [K] (int32) to tensors of their shapes; a ``phase`` without the first two launches reads them
    instead, and takes None for ``part_status`` and the twists.  ``joints``: None, or a dict of part_a, part_b [J] (int32), count ([1] int32 or None), anchor [J, 3],
    omega, velocity [J, A, 3] (float64) and the tree parent, joint_of [K] (int32).  ``points``: None, or a dict of xyz [n, 3]
    (fp32), labels [n] (int32), count ([1] int32 or None), jacobian ([n, A, 3] fp32 or None) and posed [M, n, 3] (fp32), which
    is written.  ``phase`` / ``workspace`` (float64, ``field_pose_workspace`` elements): run the launches one by one on a
    workspace of the caller's, to time them apart; FIELD_POSE_STAGED / FIELD_POSE_WIDE select the other forms of the points
    launch."""
    k = parts.numel()
    if commands.dim() != 2:
        raise ValueError("njf_hip: field_pose needs commands [M, A]")
    m, a = commands.shape
    links = bool(phase & FIELD_POSE_LINKS)   # only the links launch reads the twists: the others take None for them
    if links or omega is not None:
        if omega.dim() != 3 or tuple(omega.shape) != (k, a, 3) or velocity.shape != omega.shape:
            raise ValueError(f"njf_hip: field_pose needs omega and velocity [K, {a}, 3]")
        if part_status.numel() != k or centroid.numel() != 3 * k:
            raise ValueError("njf_hip: field_pose needs one status and one centroid per part")
    sizes = dict(rotation=9 * m * k, translation=3 * m * k, status=k, depth=k)
    for name, size in sizes.items():
        if out[name].numel() != size:
            raise ValueError(f"njf_hip: field_pose output {name} must hold {size} elements (got {out[name].numel()})")
    one = [("parts_count", parts_count)]
    j = 0
    if joints is not None:
        j = joints["part_a"].numel()
        if joints["part_b"].numel() != j or joints["anchor"].numel() != 3 * j or joints["omega"].numel() != 3 * a * j or \
                joints["velocity"].numel() != 3 * a * j or joints["parent"].numel() != k or joints["joint_of"].numel() != k:
            raise ValueError("njf_hip: field_pose needs part_a, part_b [J], anchor [J, 3], omega, velocity [J, A, 3] of the "
                             "joints and parent, joint_of [K]")
        one.append(("joints count", joints.get("count")))
    n = 0
    if points is not None:
        n = points["labels"].numel()
        jac = points.get("jacobian")
        if points["xyz"].numel() != 3 * n or points["posed"].numel() != 3 * m * n or (jac is not None and jac.numel() != 3 * a * n):
            raise ValueError("njf_hip: field_pose needs xyz [n, 3], labels [n], jacobian [n, A, 3] or None and posed [M, n, 3]")
        one.append(("count", points.get("count")))
    for name, t in one:
        if t is not None and t.numel() != 1:
            raise ValueError(f"njf_hip: field_pose {name} must hold one int32")
    if workspace is None and phase & (FIELD_POSE_LINKS | FIELD_POSE_CHAIN):
        workspace = torch.empty(field_pose_workspace(m, k), dtype=torch.float64, device=commands.device)
    jt = (lambda key, ptr=_double_ptr: None if joints is None else ptr(joints.get(key), "joints " + key))   # noqa: E731
    pt = (lambda key, ptr=_ptr: None if points is None else ptr(points.get(key), key))                       # noqa: E731
    _launch("njf_field_pose", load_library().njf_field_pose, _int32_ptr(parts, "parts"), _int32_ptr(parts_count, "parts_count"),
            int(k), _int32_ptr(part_status, "part_status"), _double_ptr(centroid, "centroid"), _double_ptr(omega, "omega"),
            _double_ptr(velocity, "velocity"), int(a), jt("part_a", _int32_ptr), jt("part_b", _int32_ptr),
            jt("count", _int32_ptr), int(j), jt("anchor"), jt("omega"), jt("velocity"), jt("parent", _int32_ptr),
            jt("joint_of", _int32_ptr), _ptr(commands, "commands"), int(m), _double_ptr(out["rotation"], "rotation"),
            _double_ptr(out["translation"], "translation"), _int32_ptr(out["status"], "status"),
            _int32_ptr(out["depth"], "depth"), pt("xyz"), pt("labels", _int32_ptr), pt("count", _int32_ptr), int(n),
            pt("jacobian"), pt("posed"), _double_ptr(workspace, "workspace"), 0 if workspace is None else int(workspace.numel()),
            int(phase))


# ---- inverse kinematics on the part tree: commands from 3-D point targets (include/njf_hip.h: njf_field_commands) ------------
FIELD_COMMANDS_MOMENTS, FIELD_COMMANDS_SOLVE = 1, 2    # NJF_FIELD_COMMANDS_MOMENTS (two launches), _SOLVE (one)
FIELD_COMMANDS_PHASES = (FIELD_COMMANDS_MOMENTS, FIELD_COMMANDS_SOLVE)
FIELD_COMMANDS_PHASE_NAMES = ("moments", "solve")
FIELD_COMMANDS_ALL = 3                                 # NJF_FIELD_COMMANDS_ALL
FIELD_COMMANDS_MOMENTS_PER_PART = 23                   # NJF_FIELD_COMMANDS_MOMENTS_PER_PART
FIELD_COMMANDS_MAX_ITERATIONS = 1000                   # NJF_FIELD_COMMANDS_MAX_ITERATIONS
FIELD_COMMANDS_NO_ROWS, FIELD_COMMANDS_NOT_FINITE = 1, 2   # status bits


def field_commands_workspace(problems: int, parts: int, action_dim: int, rows: int) -> int:
    """Doubles of workspace njf_field_commands needs: NJF_FIELD_COMMANDS_WORKSPACE(M, K, A, n) -- the chunks' partial moments
    [chunks, K, M, 23] and the twists of the links and the chains [M, 2, K, A, 6]."""
    chunks = (rows + FIELD_TWISTS_CHUNK - 1) // FIELD_TWISTS_CHUNK
    return (FIELD_COMMANDS_MOMENTS_PER_PART * chunks + 12 * action_dim) * problems * parts


def field_commands(parts: torch.Tensor, part_status: torch.Tensor, centroid: torch.Tensor, omega: torch.Tensor,
                   velocity: torch.Tensor, points: dict, out: dict, parts_count=None, joints: Optional[dict] = None,
                   weights: Optional[torch.Tensor] = None, init=None, lower=None, upper=None, reg: float = 0.0,
                   iterations: int = 20, damping: float = 1e-3, phase: int = FIELD_COMMANDS_ALL,
                   workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_commands on the part list and twists of ``field_pose``, the ``joints`` dict of ``field_pose`` (or None) and
    ``points``: a dict of xyz [n, 3] (fp32), labels [n] (int32), count ([1] int32 or None) and targets [M, n, 3] (fp32).
    ``weights``: None, [n] or [M, n] (fp32); ``init``, ``lower``, ``upper``: None or [M, A] (fp32).  ``out`` maps commands [M, A]
    (fp32), cost, initial_cost, weight [M], gradient [M, A], moments [M, K, 23] (float64), steps, status [M], part_status, depth
    [K] (int32) to tensors of their shapes.  ``phase``: FIELD_COMMANDS_MOMENTS writes moments, part_status and depth;
    FIELD_COMMANDS_SOLVE READS moments and writes everything else, part_status and depth (the same values) included; ``workspace``: float64, ``field_commands_workspace``
    elements."""
    _field_commands("field_commands", False, parts, part_status, centroid, omega, velocity, points, out, parts_count, joints, weights, init,
                    lower, upper, reg, iterations, damping, phase, workspace)


def _field_commands(entry, metric, parts, part_status, centroid, omega, velocity, points, out, parts_count, joints, weights, init, lower,
                    upper, reg, iterations, damping, phase, workspace) -> None:
    """``field_commands`` and ``field_commands_metric``: the shape checks and the call."""
    per_part = FIELD_COMMANDS_METRIC_MOMENTS_PER_PART if metric else FIELD_COMMANDS_MOMENTS_PER_PART
    information = points.get("information") if metric else None
    k = parts.numel()
    targets = points["targets"]
    if targets.dim() != 3 or targets.shape[2] != 3:
        raise ValueError(f"njf_hip: {entry} needs targets [M, n, 3]")
    m, n = targets.shape[:2]
    if omega.dim() != 3 or omega.shape[0] != k or omega.shape[2] != 3 or velocity.shape != omega.shape:
        raise ValueError(f"njf_hip: {entry} needs omega and velocity [K, A, 3]")
    a = omega.shape[1]
    if part_status.numel() != k or centroid.numel() != 3 * k:
        raise ValueError(f"njf_hip: {entry} needs one status and one centroid per part")
    if points["xyz"].numel() != 3 * n or points["labels"].numel() != n:
        raise ValueError(f"njf_hip: {entry} needs xyz [n, 3] and labels [n]")
    sizes = dict(commands=m * a, cost=m, initial_cost=m, weight=m, gradient=m * a, moments=m * k * per_part,
                 steps=m, status=m, part_status=k, depth=k)
    for name, size in sizes.items():
        if out[name].numel() != size:
            raise ValueError(f"njf_hip: {entry} output {name} must hold {size} elements (got {out[name].numel()})")
    information_per_problem = 0
    if metric:
        if information is None or tuple(information.shape) not in ((n, 6), (m, n, 6)):
            raise ValueError(f"njf_hip: {entry} needs information [n, 6] or [M, n, 6]")
        information_per_problem = int(information.dim() == 3)
    per_problem = 0
    if weights is not None:
        if tuple(weights.shape) not in ((n,), (m, n)):
            raise ValueError(f"njf_hip: {entry} needs weights [n] or [M, n]")
        per_problem = int(weights.dim() == 2)
    for name, t in (("init", init), ("lower", lower), ("upper", upper)):
        if t is not None and t.numel() != m * a:
            raise ValueError(f"njf_hip: {entry} needs {name} [M, A]")
    one = [("parts_count", parts_count), ("count", points.get("count"))]
    j = 0
    if joints is not None:
        j = joints["part_a"].numel()
        if joints["part_b"].numel() != j or joints["anchor"].numel() != 3 * j or joints["omega"].numel() != 3 * a * j or \
                joints["velocity"].numel() != 3 * a * j or joints["parent"].numel() != k or joints["joint_of"].numel() != k:
            raise ValueError(f"njf_hip: {entry} needs part_a, part_b [J], anchor [J, 3], omega, velocity [J, A, 3] of the "
                             "joints and parent, joint_of [K]")
        one.append(("joints count", joints.get("count")))
    for name, t in one:
        if t is not None and t.numel() != 1:
            raise ValueError(f"njf_hip: {entry} {name} must hold one int32")
    if workspace is None:
        workspace = torch.empty((field_commands_metric_workspace if metric else field_commands_workspace)(m, k, a, n),
                                dtype=torch.float64, device=targets.device)
    jt = (lambda key, ptr=_double_ptr: None if joints is None else ptr(joints.get(key), "joints " + key))   # noqa: E731
    rows = [_ptr(targets, "targets")] + ([_ptr(information, "information"), information_per_problem] if metric else [])
    _launch("njf_" + entry, getattr(load_library(), "njf_" + entry), _int32_ptr(parts, "parts"),
            _int32_ptr(parts_count, "parts_count"), int(k), _int32_ptr(part_status, "part_status"), _double_ptr(centroid, "centroid"),
            _double_ptr(omega, "omega"), _double_ptr(velocity, "velocity"), int(a), jt("part_a", _int32_ptr), jt("part_b", _int32_ptr),
            jt("count", _int32_ptr), int(j), jt("anchor"), jt("omega"), jt("velocity"), jt("parent", _int32_ptr),
            jt("joint_of", _int32_ptr), _ptr(points["xyz"], "xyz"), _int32_ptr(points["labels"], "labels"),
            _int32_ptr(points.get("count"), "count"), int(n), *rows, int(m), _ptr(weights, "weights"), per_problem,
            _ptr(init, "init"), _ptr(lower, "lower"), _ptr(upper, "upper"), float(reg), int(iterations), float(damping),
            _ptr(out["commands"], "commands"), _double_ptr(out["cost"], "cost"), _double_ptr(out["initial_cost"], "initial_cost"),
            _double_ptr(out["weight"], "weight"), _int32_ptr(out["steps"], "steps"), _double_ptr(out["gradient"], "gradient"),
            _int32_ptr(out["status"], "status"), _int32_ptr(out["part_status"], "part_status"), _int32_ptr(out["depth"], "depth"),
            _double_ptr(out["moments"], "moments"), _double_ptr(workspace, "workspace"), int(workspace.numel()), int(phase))


# ---- the same with a 3 x 3 information per target (include/njf_hip.h: njf_field_commands_metric) ------------------------------
FIELD_COMMANDS_METRIC_MOMENTS_PER_PART = 74            # NJF_FIELD_COMMANDS_METRIC_MOMENTS_PER_PART
FIELD_COMMANDS_METRIC_BUTTERFLY = 4                    # NJF_FIELD_COMMANDS_METRIC_BUTTERFLY: the moments by 74 butterflies


def field_commands_metric_workspace(problems: int, parts: int, action_dim: int, rows: int) -> int:
    """Doubles of workspace njf_field_commands_metric needs: NJF_FIELD_COMMANDS_METRIC_WORKSPACE(M, K, A, n) -- the chunks'
    partial moments [chunks, K, M, 74] and the twists of the links and the chains [M, 2, K, A, 6]."""
    chunks = (rows + FIELD_TWISTS_CHUNK - 1) // FIELD_TWISTS_CHUNK
    return (FIELD_COMMANDS_METRIC_MOMENTS_PER_PART * chunks + 12 * action_dim) * problems * parts


def field_commands_metric(parts: torch.Tensor, part_status: torch.Tensor, centroid: torch.Tensor, omega: torch.Tensor,
                          velocity: torch.Tensor, points: dict, out: dict, parts_count=None, joints: Optional[dict] = None,
                          weights: Optional[torch.Tensor] = None, init=None, lower=None, upper=None, reg: float = 0.0,
                          iterations: int = 20, damping: float = 1e-3, phase: int = FIELD_COMMANDS_ALL,
                          workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_commands_metric: ``field_commands`` with ``points["information"]`` [n, 6] or [M, n, 6] (fp32), the symmetric
    3 x 3 information of every target as [xx xy xz yy yz zz]; ``out["moments"]`` is [M, K, 74].  ``phase`` may add
    FIELD_COMMANDS_METRIC_BUTTERFLY to the moments phase; ``workspace``: float64, ``field_commands_metric_workspace`` elements."""
    _field_commands("field_commands_metric", True, parts, part_status, centroid, omega, velocity, points, out, parts_count, joints,
                    weights, init, lower, upper, reg, iterations, damping, phase, workspace)


# ---- closest points of an unlabelled cloud against a cell list (include/njf_hip.h: njf_field_nearest) ------------------------
FIELD_NEAREST_BUILD, FIELD_NEAREST_QUERY = 1, 2        # NJF_FIELD_NEAREST_BUILD (a memset, five launches), _QUERY (a memset, one)
FIELD_NEAREST_PHASES = (FIELD_NEAREST_BUILD, FIELD_NEAREST_QUERY)
FIELD_NEAREST_PHASE_NAMES = ("build", "query")
FIELD_NEAREST_ALL = 3                                  # NJF_FIELD_NEAREST_ALL
FIELD_NEAREST_WAVE = 4                                 # NJF_FIELD_NEAREST_WAVE: the query launch with a wave per query
FIELD_NEAREST_MAX_RINGS = 64                           # NJF_FIELD_NEAREST_MAX_RINGS
FIELD_NEAREST_MAX_DIM = 1024                           # NJF_FIELD_NEAREST_MAX_DIM


def field_nearest_workspace(observed: int, cells: int, points: int) -> int:
    """32-bit words of workspace njf_field_nearest needs: NJF_FIELD_NEAREST_WORKSPACE(Mo, C, T) -- Mo (C + 1) starts, Mo C
    cursors, 4 Mo T record words and 3 words of alignment."""
    return observed * (2 * cells + 1 + 4 * points) + 3


def _cloud_shape(op: str, name: str, layout: str, cloud) -> tuple:
    """(M, T) of ``cloud``: a tensor [M, T, 3], or the shape tuple that stands for it in a phase that does not read it."""
    if not torch.is_tensor(cloud):
        return tuple(int(v) for v in cloud)
    if cloud.dim() != 3 or cloud.shape[2] != 3:
        raise ValueError(f"njf_hip: {op} needs {name} [{layout}, 3]")
    return int(cloud.shape[0]), int(cloud.shape[1])


def _posed_rows(op: str, points, count, labels, name: str = "points") -> tuple:
    """(Mq, n) of the posed rows ``points`` [Mq, n, 3] (or the shape tuple that stands for them) with ``count`` [1] and ``labels``
    [n], each int32 or None."""
    mq, n = _cloud_shape(op, name, "Mq, n", points)
    if count is not None and count.numel() != 1:
        raise ValueError(f"njf_hip: {op} count must hold one int32")
    if labels is not None and labels.numel() != n:
        raise ValueError(f"njf_hip: {op} needs labels [n]")
    return mq, n


def _view_count(op: str, k, w2c, views: Optional[int] = None) -> int:
    """V of the cameras ``k`` [V, 3, 3] and ``w2c`` [V, 4, 4]; ``views``: the V they must have, where the caller knows one."""
    v, shown = (int(k.shape[0]) if k.dim() else -1, "V") if views is None else (views, views)
    if tuple(k.shape) != (v, 3, 3) or tuple(w2c.shape) != (v, 4, 4):
        raise ValueError(f"njf_hip: {op} needs k [{shown}, 3, 3] and w2c [{shown}, 4, 4]")
    return v


def _check_output_sizes(op: str, out: dict, sizes: dict) -> None:
    for name, size in sizes.items():
        if out[name].numel() != size:
            raise ValueError(f"njf_hip: {op} output {name} must hold {size} elements (got {out[name].numel()})")


def _cell_list_workspace(words, grid: FieldGrid, clouds: int, points: int, device) -> torch.Tensor:
    """A fresh workspace of ``words(clouds, cells of the grid, points)`` int32 elements."""
    cells = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
    return torch.empty(words(clouds, cells, points), dtype=torch.int32, device=device)


def field_nearest(observed: Optional[torch.Tensor], queries: Optional[torch.Tensor], grid: FieldGrid, max_distance: float, out: dict,
                  problems: int, observed_count=None, count=None, labels=None, phase: int = FIELD_NEAREST_ALL,
                  workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_nearest on ``observed`` [Mo, T, 3] and ``queries`` [Mq, n, 3] (fp32) for ``problems`` = M problems, Mo and Mq
    each 1 or M, against the cell lattice ``grid``.  ``observed_count`` [Mo], ``count`` [1], ``labels`` [n]: int32 or None.
    ``out`` maps index [M, n] (int32), distance2 [M, n], matched [M, n, 3] (fp32) and found [M] (int32) to tensors of their
    shapes.  ``phase``: FIELD_NEAREST_BUILD reads ``observed`` and writes the workspace, FIELD_NEAREST_QUERY reads the workspace
    and writes ``out``; a phase without the build takes the SHAPE ``(Mo, T)`` for ``observed``, one without the query the shape
    ``(Mq, n)`` for ``queries`` and None for ``out``.  ``workspace``: int32, ``field_nearest_workspace`` elements."""
    mo, t = _cloud_shape("field_nearest", "observed", "Mo, T", observed)
    (mq, n), m = _posed_rows("field_nearest", queries, count, labels, "queries"), int(problems)
    build, query = bool(phase & FIELD_NEAREST_BUILD), bool(phase & FIELD_NEAREST_QUERY)
    if (build and not torch.is_tensor(observed)) or (query and not torch.is_tensor(queries)):
        raise ValueError("njf_hip: field_nearest needs the observed points to build and the queries to query")
    if observed_count is not None and observed_count.numel() != mo:
        raise ValueError("njf_hip: field_nearest needs observed_count [Mo]")
    if query:
        _check_output_sizes("field_nearest", out, dict(index=m * n, distance2=m * n, matched=3 * m * n, found=m))
    if workspace is None:
        workspace = _cell_list_workspace(field_nearest_workspace, grid, mo, t, (observed if build else queries).device)
    o = (lambda key, ptr: ptr(out[key], key) if query else None)   # noqa: E731
    _launch("njf_field_nearest", load_library().njf_field_nearest, _ptr(observed, "observed") if build else None,
            _int32_ptr(observed_count, "observed_count"), mo, t, _ptr(queries, "queries") if query else None,
            _int32_ptr(count, "count"), _int32_ptr(labels, "labels"), mq, n, m, C.byref(grid), float(max_distance),
            o("index", _int32_ptr), o("distance2", _ptr), o("matched", _ptr), o("found", _int32_ptr),
            _int32_ptr(workspace, "workspace"), int(workspace.numel()), int(phase))


# ---- surface normals of an observed cloud from integer moments on the cell list (include/njf_hip.h: njf_field_normals) --------
FIELD_NORMALS_BUILD, FIELD_NORMALS_MOMENTS, FIELD_NORMALS_FINISH = 1, 2, 4   # NJF_FIELD_NORMALS_BUILD (nearest's), _MOMENTS, _FINISH
FIELD_NORMALS_PHASES = (FIELD_NORMALS_BUILD, FIELD_NORMALS_MOMENTS, FIELD_NORMALS_FINISH)
FIELD_NORMALS_PHASE_NAMES = ("build", "moments", "finish")
FIELD_NORMALS_ALL = 7                                  # NJF_FIELD_NORMALS_ALL
FIELD_NORMALS_WAVE = 8                                 # NJF_FIELD_NORMALS_WAVE: the moments launch with a wave per row
FIELD_NORMALS_MOMENTS_PER_ROW = 10                     # NJF_FIELD_NORMALS_MOMENTS_PER_ROW: S0, S1[3], S2[6]
FIELD_NORMALS_SWEEPS = 8                               # NJF_FIELD_NORMALS_SWEEPS
FIELD_NORMALS_MAX_POINTS = 2 ** 26                     # T below this: the int64 second moments cannot overflow
field_normals_workspace = field_nearest_workspace      # NJF_FIELD_NORMALS_WORKSPACE: the cell list is njf_field_nearest's


def field_normals(observed: Optional[torch.Tensor], queries: Optional[torch.Tensor], grid: FieldGrid, radius: float, out: dict,
                  problems: int, observed_count=None, count=None, viewpoint=None, min_neighbours: int = 3,
                  phase: int = FIELD_NORMALS_ALL, workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_normals on ``observed`` [Mo, T, 3] and ``queries`` [Mq, n, 3] (fp32) for ``problems`` = M problems, Mo and Mq
    each 1 or M, against the cell lattice ``grid``.  ``observed_count`` [Mo], ``count`` [1]: int32 or None; ``viewpoint`` [Mv,
    3] fp32 or None, Mv 1 or M.  ``out`` maps moments [M, n, 10] (int64), normal [M, n, 3], variation [M, n] (fp32), neighbours
    [M, n] (int32) and -- optionally -- eigenvalues [M, n, 3] (float64) to tensors of their shapes.  ``phase``:
    FIELD_NORMALS_BUILD reads ``observed`` and writes the workspace (njf_field_nearest's build), FIELD_NORMALS_MOMENTS reads the
    workspace and the queries and writes ``out["moments"]`` [+ FIELD_NORMALS_WAVE], FIELD_NORMALS_FINISH reads the moments and
    writes the other outputs; a phase without the build takes the SHAPE ``(Mo, T)`` for ``observed``.  ``workspace``: int32,
    ``field_normals_workspace`` elements, not needed by the finish alone."""
    mo, t = _cloud_shape("field_normals", "observed", "Mo, T", observed)
    (mq, n), m = _posed_rows("field_normals", queries, count, None, "queries"), int(problems)
    build, sums, finish = (bool(phase & p) for p in FIELD_NORMALS_PHASES)
    if (build and not torch.is_tensor(observed)) or ((sums or finish) and not torch.is_tensor(queries)):
        raise ValueError("njf_hip: field_normals needs the observed points to build and the queries for the moments and the finish")
    if observed_count is not None and observed_count.numel() != mo:
        raise ValueError("njf_hip: field_normals needs observed_count [Mo]")
    if viewpoint is not None and (viewpoint.dim() != 2 or viewpoint.shape[1] != 3):
        raise ValueError("njf_hip: field_normals needs viewpoint [Mv, 3]")
    sizes = dict(moments=10 * m * n) if sums or finish else {}
    if finish:
        sizes.update(normal=3 * m * n, neighbours=m * n, variation=m * n)
        if out.get("eigenvalues") is not None:
            sizes.update(eigenvalues=3 * m * n)
    _check_output_sizes("field_normals", out, sizes)
    if workspace is None and (build or sums):
        workspace = _cell_list_workspace(field_normals_workspace, grid, mo, t, (observed if build else queries).device)
    o = (lambda key, ptr, *dtype: ptr(out[key], key, *dtype) if key in sizes else None)   # noqa: E731
    _launch("njf_field_normals", load_library().njf_field_normals, _ptr(observed, "observed") if build else None,
            _int32_ptr(observed_count, "observed_count"), mo, t, _ptr(queries, "queries") if sums or finish else None,
            _int32_ptr(count, "count"), mq, n, m, C.byref(grid), float(radius), int(min_neighbours),
            _ptr(viewpoint, "viewpoint"), 0 if viewpoint is None else int(viewpoint.shape[0]), o("moments", _ptr, torch.int64),
            o("normal", _ptr), o("neighbours", _int32_ptr), o("variation", _ptr), o("eigenvalues", _double_ptr),
            _int32_ptr(workspace, "workspace"), 0 if workspace is None else int(workspace.numel()), int(phase))


# ---- a depth frame to world points (include/njf_hip.h: njf_field_depth_points) -------------------------------------------------------
FIELD_DEPTH_RAY, FIELD_DEPTH_Z = 0, 1                  # NJF_FIELD_DEPTH_RAY (t = depth), NJF_FIELD_DEPTH_Z (t = depth / cz)
FIELD_DEPTH_KINDS = {"ray": FIELD_DEPTH_RAY, "z": FIELD_DEPTH_Z}


def field_depth_points(depth: torch.Tensor, k_inv: torch.Tensor, c2w: torch.Tensor, kind: int, near: float, far: float,
                       max_jump: float, views_per_scene: int, points: torch.Tensor, kept: torch.Tensor) -> None:
    """njf_field_depth_points on ``depth`` [B, H, W], ``k_inv`` [B, 3, 3] (the INVERSE intrinsics) and ``c2w`` [B, 4, 4] (fp32):
    ``points`` [B / V, V*H*W, 3] (fp32) and ``kept`` [B / V] (int32), every row written.  ``max_jump`` 0 = no flying-pixel test."""
    if depth.dim() != 3:
        raise ValueError("njf_hip: field_depth_points needs depth [B, H, W]")
    b, h, w = (int(v) for v in depth.shape)
    views = int(views_per_scene)
    if views < 1 or b % views:
        raise ValueError(f"njf_hip: field_depth_points needs B a multiple of views_per_scene (got {b} and {views_per_scene})")
    for name, t, size in (("k_inv", k_inv, 9 * b), ("c2w", c2w, 16 * b), ("points", points, 3 * b * h * w), ("kept", kept, b // views)):
        if t.numel() != size:
            raise ValueError(f"njf_hip: field_depth_points {name} must hold {size} elements (got {t.numel()})")
    _launch("njf_field_depth_points", load_library().njf_field_depth_points, _ptr(depth, "depth"), b, h, w, _ptr(k_inv, "k_inv"),
            _ptr(c2w, "c2w"), int(kind), float(near), float(far), float(max_jump), views, _ptr(points, "points"),
            _int32_ptr(kept, "kept"))


# ---- one centroid per occupied cell of a cloud (include/njf_hip.h: njf_field_voxels) --------------------------------------------------
FIELD_VOXELS_BUILD, FIELD_VOXELS_REDUCE, FIELD_VOXELS_COMPACT = 1, 2, 4   # NJF_FIELD_VOXELS_BUILD (nearest's), _REDUCE, _COMPACT
FIELD_VOXELS_PHASES = (FIELD_VOXELS_BUILD, FIELD_VOXELS_REDUCE, FIELD_VOXELS_COMPACT)
FIELD_VOXELS_PHASE_NAMES = ("build", "reduce", "compact")
FIELD_VOXELS_ALL = 7                                   # NJF_FIELD_VOXELS_ALL
FIELD_VOXELS_WAVE = 8                                  # NJF_FIELD_VOXELS_WAVE: the reduce launch with a wave per cell
FIELD_VOXELS_QUANTUM = 2 ** 20                         # NJF_FIELD_VOXELS_QUANTUM: steps per cell of the integer sums


def field_voxels_workspace(problems: int, cells: int, points: int) -> int:
    """32-bit words of workspace njf_field_voxels needs: NJF_FIELD_VOXELS_WORKSPACE(M, C, T) -- njf_field_nearest's and, behind
    it, 3 M C int64 sums, M C counts and M C + 1 second starts."""
    return field_nearest_workspace(problems, cells, points) + 8 * problems * cells + 1


def field_voxels(points, grid: FieldGrid, out: dict, points_count=None, min_points: int = 1, phase: int = FIELD_VOXELS_ALL,
                 workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_voxels on ``points`` [M, T, 3] (fp32) against the cell lattice ``grid``; ``points_count`` [M]: int32 or None.
    ``out`` maps points [M, capacity, 3] (fp32), weight, cell [M, capacity] (int32), sums [M, capacity, 3] (int64), count and
    outside [M] (int32) to tensors of their shapes; the capacity is read off ``out["weight"]``.  ``phase``: FIELD_VOXELS_BUILD
    reads ``points`` and writes the workspace (njf_field_nearest's build), FIELD_VOXELS_REDUCE [+ FIELD_VOXELS_WAVE] reads the
    cell list and writes the per-cell sums and ``out["outside"]``, FIELD_VOXELS_COMPACT writes the other outputs; a phase
    without the build takes the SHAPE ``(M, T)`` for ``points``.  ``workspace``: int32, ``field_voxels_workspace`` elements."""
    m, t = _cloud_shape("field_voxels", "points", "M, T", points)
    build = bool(phase & FIELD_VOXELS_BUILD)
    if build and not torch.is_tensor(points):
        raise ValueError("njf_hip: field_voxels needs the points to build")
    if points_count is not None and points_count.numel() != m:
        raise ValueError("njf_hip: field_voxels needs points_count [M]")
    if out["weight"].dim() != 2 or out["weight"].shape[0] != m or out["weight"].shape[1] < 1:
        raise ValueError("njf_hip: field_voxels needs weight [M, capacity] with capacity >= 1")
    capacity = int(out["weight"].shape[1])
    _check_output_sizes("field_voxels", out, dict(points=3 * m * capacity, weight=m * capacity, cell=m * capacity,
                                                  sums=3 * m * capacity, count=m, outside=m))
    if workspace is None:
        workspace = _cell_list_workspace(field_voxels_workspace, grid, m, t, out["weight"].device)
    _launch("njf_field_voxels", load_library().njf_field_voxels, _ptr(points, "points") if build else None,
            _int32_ptr(points_count, "points_count"), m, t, C.byref(grid), int(min_points), capacity, _ptr(out["points"], "points"),
            _int32_ptr(out["weight"], "weight"), _int32_ptr(out["cell"], "cell"), _ptr(out["sums"], "sums", torch.int64),
            _int32_ptr(out["count"], "count"), _int32_ptr(out["outside"], "outside"), _int32_ptr(workspace, "workspace"),
            int(workspace.numel()), int(phase))


# ---- which posed rows a depth camera sees: a z-buffer of points (include/njf_hip.h: njf_field_visible) -------------------------------
FIELD_VISIBLE_SPLAT, FIELD_VISIBLE_RESOLVE, FIELD_VISIBLE_TEST = 1, 2, 4   # NJF_FIELD_VISIBLE_SPLAT, _RESOLVE, _TEST: a memset, a launch
FIELD_VISIBLE_PHASES = (FIELD_VISIBLE_SPLAT, FIELD_VISIBLE_RESOLVE, FIELD_VISIBLE_TEST)
FIELD_VISIBLE_PHASE_NAMES = ("splat", "resolve", "test")
FIELD_VISIBLE_ALL = 7                                  # NJF_FIELD_VISIBLE_ALL
FIELD_VISIBLE_DIRECT = 8                               # NJF_FIELD_VISIBLE_DIRECT: the splat without the load before the atomic
FIELD_VISIBLE_MAX_VIEWS = 32                           # NJF_FIELD_VISIBLE_MAX_VIEWS: one bit of `seen` per view
FIELD_VISIBLE_MAX_FOOTPRINT = 4                        # NJF_FIELD_VISIBLE_MAX_FOOTPRINT
FIELD_VISIBLE_OUTPUTS = (("depth", torch.float32), ("index", torch.int32), ("covered", torch.int32), ("seen", torch.int32),
                         ("culled", torch.float32), ("visible", torch.int32), ("pixel", torch.int32), ("z", torch.float32))


def field_visible_workspace(m: int, v: int, h: int, w: int) -> int:
    """32-bit words of workspace njf_field_visible needs: NJF_FIELD_VISIBLE_WORKSPACE(M, V, H, W) -- M V H W keys of 8 bytes and
    one word of alignment."""
    return 2 * m * v * h * w + 1


def field_visible_default_phase() -> int:
    """FIELD_VISIBLE_ALL in the default form of the splat; ``NJF_FIELD_VISIBLE_DIRECT=1`` in the environment selects the form
    without the load before the atomic (equal bytes: DESIGN.md section 24 holds the measurement)."""
    return FIELD_VISIBLE_ALL | (FIELD_VISIBLE_DIRECT if os.environ.get("NJF_FIELD_VISIBLE_DIRECT", "0") == "1" else 0)


def field_visible(points: torch.Tensor, k: torch.Tensor, w2c: torch.Tensor, height: int, width: int, out: dict, problems: int,
                  count=None, labels=None, footprint: int = 1, near: float = 0.0, tolerance: float = 0.01,
                  phase: int = FIELD_VISIBLE_ALL, workspace: Optional[torch.Tensor] = None) -> None:
    """njf_field_visible on ``points`` [Mq, n, 3] (fp32) for ``problems`` = M problems, Mq 1 or M, through the cameras ``k`` [V, 3,
    3] (normalised intrinsics) and ``w2c`` [V, 4, 4] (fp32) into images of ``height`` x ``width``.  ``count`` [1], ``labels`` [n]:
    int32 or None.  ``out`` maps depth, index [M, V, H, W], covered [M, V], seen [M, n], culled [M, n, 3], visible [M], pixel and z
    [M, V, n] (FIELD_VISIBLE_OUTPUTS holds the element types) to tensors of their shapes.  ``phase``: FIELD_VISIBLE_SPLAT [+
    FIELD_VISIBLE_DIRECT] reads the points and writes the workspace, FIELD_VISIBLE_RESOLVE writes depth, index and covered from
    it, FIELD_VISIBLE_TEST reads the points and ``out["depth"]`` and writes the other five.  ``workspace``: int32,
    ``field_visible_workspace`` elements."""
    mq, n = _posed_rows("field_visible", points, count, labels)
    m, v, h, w = int(problems), _view_count("field_visible", k, w2c), int(height), int(width)
    splat, resolve, test = (bool(phase & p) for p in FIELD_VISIBLE_PHASES)
    sizes = {}
    if resolve or test:
        sizes.update(depth=m * v * h * w)
    if resolve:
        sizes.update(index=m * v * h * w, covered=m * v)
    if test:
        sizes.update(seen=m * n, culled=3 * m * n, visible=m, pixel=m * v * n, z=m * v * n)
    _check_output_sizes("field_visible", out, sizes)
    if workspace is None and (splat or resolve):
        workspace = torch.empty(field_visible_workspace(m, v, h, w), dtype=torch.int32, device=points.device)
    o = (lambda key, ptr: ptr(out[key], key) if key in sizes else None)   # noqa: E731
    _launch("njf_field_visible", load_library().njf_field_visible, _ptr(points, "points"), _int32_ptr(count, "count"),
            _int32_ptr(labels, "labels"), mq, n, m, _ptr(k, "k"), _ptr(w2c, "w2c"), v, h, w, int(footprint), float(near),
            float(tolerance), o("depth", _ptr), o("index", _int32_ptr), o("covered", _int32_ptr), o("seen", _int32_ptr),
            o("culled", _ptr), o("visible", _int32_ptr), o("pixel", _int32_ptr), o("z", _ptr),
            _int32_ptr(workspace, "workspace"), 0 if workspace is None else int(workspace.numel()), int(phase))


# ---- posed rows against a depth frame by projection (include/njf_hip.h: njf_field_frame) ----------------------------------------------
FIELD_FRAME_MATCH = 1                                  # NJF_FIELD_FRAME_MATCH: two memsets and one launch
FIELD_FRAME_KEEP_HIDDEN = 2                            # NJF_FIELD_FRAME_KEEP_HIDDEN: BEHIND rows are searched too
FIELD_FRAME_MAX_REACH = 8                              # NJF_FIELD_FRAME_MAX_REACH
FIELD_FRAME_STATE_NAMES = ("outside", "no_return", "in_front", "on", "behind")   # NJF_FIELD_FRAME_OUTSIDE .. _BEHIND = 0 .. 4
FIELD_FRAME_OUTSIDE, FIELD_FRAME_NO_RETURN, FIELD_FRAME_IN_FRONT, FIELD_FRAME_ON, FIELD_FRAME_BEHIND = range(5)
FIELD_FRAME_STATES = 5                                 # NJF_FIELD_FRAME_STATES
FIELD_FRAME_OUTPUTS = (("pixel", torch.int32), ("z", torch.float32), ("state", torch.int32), ("index", torch.int32),
                       ("distance2", torch.float32), ("matched", torch.float32), ("found", torch.int32), ("states", torch.int32))


def field_frame(points: torch.Tensor, frame: torch.Tensor, k: torch.Tensor, w2c: torch.Tensor, height: int, width: int,
                max_distance: float, out: dict, problems: int, count=None, labels=None, reach: int = 4, near: float = 0.0,
                tolerance: float = 0.02, phase: int = FIELD_FRAME_MATCH) -> None:
    """njf_field_frame on ``points`` [Mq, n, 3] and the organised cloud ``frame`` [Mo, V * H * W, 3] (fp32) for ``problems`` = M
    problems, Mq and Mo each 1 or M, through the cameras ``k`` [V, 3, 3] and ``w2c`` [V, 4, 4] (fp32) of images of ``height`` x
    ``width``.  ``count`` [1], ``labels`` [n]: int32 or None.  ``out`` maps pixel, z, state [M, V, n], index, distance2 [M, n],
    matched [M, n, 3], found [M] and states [M, 5] (FIELD_FRAME_OUTPUTS holds the element types) to tensors of their shapes.
    ``phase``: FIELD_FRAME_MATCH [+ FIELD_FRAME_KEEP_HIDDEN]."""
    mq, n = _posed_rows("field_frame", points, count, labels)
    mo, t = _cloud_shape("field_frame", "frame", "Mo, V * H * W", frame)
    m, v, h, w = int(problems), _view_count("field_frame", k, w2c), int(height), int(width)
    if t != v * h * w:
        raise ValueError(f"njf_hip: field_frame needs frame [Mo, {v * h * w}, 3] for {v} views of {h} x {w} (got {t} rows)")
    _check_output_sizes("field_frame", out, dict(pixel=m * v * n, z=m * v * n, state=m * v * n, index=m * n, distance2=m * n,
                                                 matched=3 * m * n, found=m, states=m * FIELD_FRAME_STATES))
    _launch("njf_field_frame", load_library().njf_field_frame, _ptr(points, "points"), _int32_ptr(count, "count"),
            _int32_ptr(labels, "labels"), mq, n, m, _ptr(frame, "frame"), mo, _ptr(k, "k"), _ptr(w2c, "w2c"), v, h, w, int(reach),
            float(near), float(tolerance), float(max_distance), _int32_ptr(out["pixel"], "pixel"), _ptr(out["z"], "z"),
            _int32_ptr(out["state"], "state"), _int32_ptr(out["index"], "index"), _ptr(out["distance2"], "distance2"),
            _ptr(out["matched"], "matched"), _int32_ptr(out["found"], "found"), _int32_ptr(out["states"], "states"), int(phase))


# ---- depth frames fused into a truncated signed distance, and sampled at rows (include/njf_hip.h: njf_field_tsdf) ---------------------
FIELD_TSDF_STATE_NAMES = ("outside", "unknown", "known")   # NJF_FIELD_TSDF_OUTSIDE, _UNKNOWN, _KNOWN = 0, 1, 2
FIELD_TSDF_OUTSIDE, FIELD_TSDF_UNKNOWN, FIELD_TSDF_KNOWN = range(3)
FIELD_TSDF_STATES = 3                                  # NJF_FIELD_TSDF_STATES
FIELD_TSDF_OUTPUTS = (("values", torch.float32), ("weight", torch.float32), ("known", torch.int32))
FIELD_TSDF_SAMPLE_OUTPUTS = (("state", torch.int32), ("distance", torch.float32), ("gradient", torch.float32), ("states", torch.int32))


def field_tsdf(grid: FieldGrid, depth: torch.Tensor, k: torch.Tensor, w2c: torch.Tensor, truncation: float, out: dict,
               near: float = 0.0, far: float = float("inf"), max_weight: float = float("inf"), values_in=None, weight_in=None) -> None:
    """njf_field_tsdf on ``depth`` [M, V, H, W] (fp32, camera-space z) through the cameras ``k`` [V, 3, 3] and ``w2c`` [V, 4, 4] onto
    the nodes of ``grid``.  ``out`` maps values, weight [M, N] (fp32) and known [M] (int32) to tensors of their shapes;
    ``values_in`` and ``weight_in`` [M, N]: the running state, both or neither -- they may be the outputs themselves."""
    if depth.dim() != 4:
        raise ValueError("njf_hip: field_tsdf needs depth [M, V, H, W]")
    m, v, h, w = (int(s) for s in depth.shape)
    _view_count("field_tsdf", k, w2c, v)
    nodes = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
    _check_output_sizes("field_tsdf", out, dict(values=m * nodes, weight=m * nodes, known=m))
    for name, t in (("values_in", values_in), ("weight_in", weight_in)):
        if t is not None and t.numel() != m * nodes:
            raise ValueError(f"njf_hip: field_tsdf {name} must hold {m * nodes} elements (got {t.numel()})")
    _launch("njf_field_tsdf", load_library().njf_field_tsdf, C.byref(grid), _ptr(depth, "depth"), m, v, h, w, _ptr(k, "k"),
            _ptr(w2c, "w2c"), float(near), float(far), float(truncation), float(max_weight), _ptr(values_in, "values_in"),
            _ptr(weight_in, "weight_in"), _ptr(out["values"], "values"), _ptr(out["weight"], "weight"),
            _int32_ptr(out["known"], "known"))


def field_tsdf_sample(points: torch.Tensor, grid: FieldGrid, values: torch.Tensor, weight: torch.Tensor, out: dict, problems: int,
                      count=None, labels=None) -> None:
    """njf_field_tsdf_sample on ``points`` [Mq, n, 3] (fp32) in the field ``values``, ``weight`` [Mf, N] (fp32) on ``grid`` for
    ``problems`` = M problems, Mq and Mf each 1 or M.  ``count`` [1], ``labels`` [n]: int32 or None.  ``out`` maps state, distance
    [M, n], gradient [M, n, 3] and states [M, 3] (FIELD_TSDF_SAMPLE_OUTPUTS holds the element types) to tensors of their shapes."""
    mq, n = _posed_rows("field_tsdf_sample", points, count, labels)
    m = int(problems)
    nodes = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
    if values.dim() != 2 or values.shape[1] != nodes or tuple(weight.shape) != tuple(values.shape):
        raise ValueError(f"njf_hip: field_tsdf_sample needs values and weight [Mf, {nodes}]")
    _check_output_sizes("field_tsdf_sample", out, dict(state=m * n, distance=m * n, gradient=3 * m * n, states=m * FIELD_TSDF_STATES))
    _launch("njf_field_tsdf_sample", load_library().njf_field_tsdf_sample, _ptr(points, "points"), _int32_ptr(count, "count"),
            _int32_ptr(labels, "labels"), mq, n, m, C.byref(grid), _ptr(values, "values"), _ptr(weight, "weight"),
            int(values.shape[0]), _int32_ptr(out["state"], "state"), _ptr(out["distance"], "distance"),
            _ptr(out["gradient"], "gradient"), _int32_ptr(out["states"], "states"))


def solve_action(mean_position, jacobian, projection, target_flow, visible_mask, init_action, iterations: int,
                 damping: float, action) -> None:
    """mean_position [B,R,3], jacobian [B,R,3,A], projection [B,3,4], target_flow [B,R,2] -> action [B,A]."""
    b, r = target_flow.shape[:2]
    _launch("njf_solve_action", load_library().njf_solve_action, _ptr(mean_position), _ptr(jacobian), _ptr(projection), _ptr(target_flow),
                                           _ptr(visible_mask), _ptr(init_action), b, r, jacobian.shape[-1], int(iterations),
                                           float(damping), _ptr(action))


SOLVE_MAX_ACTION_DIM = 16
SOLVE_LOSSES = {"mse": 0, "smooth_l1": 1}   # include/njf_hip.h: NJF_LOSS_*


def solve_action_robust(mean_position, jacobian, projection, target_flow, visible_mask, init_action, lower, upper,
                        views: int, loss: str, beta: float, reg: float, iterations: int, damping: float, action) -> None:
    """njf_solve_action_robust: mean_position [B,R,3], jacobian [B,R,3,A], projection [B,3,4], target_flow [B,R,2],
    visible_mask [B,R] | None, init_action / lower / upper [G,A] | None with B = G * views -> action [G,A]."""
    if loss not in SOLVE_LOSSES:
        raise ValueError(f"njf_hip: unknown loss {loss!r}; choose from {sorted(SOLVE_LOSSES)}")
    if target_flow.dim() != 3 or target_flow.shape[-1] != 2:
        raise ValueError(f"njf_hip: target_flow must be [B,R,2] (got {tuple(target_flow.shape)})")
    b, r = target_flow.shape[:2]
    a = jacobian.shape[-1]
    if views < 1 or b % views:
        raise ValueError(f"njf_hip: views_per_command={views} must be >= 1 and divide the batch of {b} linearisations")
    if not 1 <= a <= SOLVE_MAX_ACTION_DIM:
        raise ValueError(f"njf_hip: the solve supports 1 <= A <= {SOLVE_MAX_ACTION_DIM} (got {a})")
    g = b // views
    shapes = {"mean_position": (mean_position, (b, r, 3)), "jacobian": (jacobian, (b, r, 3, a)),
              "projection": (projection, (b, 3, 4)), "visible_mask": (visible_mask, (b, r)),
              "init_action": (init_action, (g, a)), "lower": (lower, (g, a)), "upper": (upper, (g, a)),
              "action": (action, (g, a))}
    for name, (t, shape) in shapes.items():
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"njf_hip: {name} must be {list(shape)} (got {list(t.shape)})")
    _launch("njf_solve_action_robust", load_library().njf_solve_action_robust, _ptr(mean_position, "mean_position"),
            _ptr(jacobian, "jacobian"), _ptr(projection, "projection"), _ptr(target_flow, "target_flow"),
            _ptr(visible_mask, "visible_mask"), _ptr(init_action, "init_action"), _ptr(lower, "lower"),
            _ptr(upper, "upper"), b, int(views), r, a, SOLVE_LOSSES[loss], float(beta), float(reg), int(iterations),
            float(damping), _ptr(action, "action"))


def scatter_footprint(grad, foot_idx, foot_w, out, run_length: int = 1) -> None:
    """out [T,S*C] += bilinear-footprint scatter of grad [P,C] or [S,P,C] (foot_idx [P,4] int32, foot_w [P,4]): the input
    gradient of the pixel-aligned sampling, see include/njf_hip.h.  A 3-D ``grad`` may be a strided view along its first
    axis (e.g. ``deltas[0:6:2]``): S gradients of the same points land side by side in ``out``'s columns, one launch.
    ``run_length``: samples per ray (consecutive points that mostly share texels are merged in registers before the
    atomics)."""
    if grad.dim() == 2:
        grad = grad.unsqueeze(0)
    slices, points, channels = grad.shape
    if grad.stride(2) != 1 or grad.stride(1) != channels:
        raise ValueError("njf_hip: scatter_footprint needs [P,C]-contiguous gradient slices")
    if tuple(foot_idx.shape) != (points, 4) or tuple(foot_w.shape) != (points, 4) or out.shape[1] != slices * channels:
        raise ValueError("njf_hip: scatter_footprint shape mismatch")
    if not out.is_contiguous():
        raise ValueError("njf_hip: scatter_footprint output must be contiguous")
    if not grad.is_cuda or grad.dtype != torch.float32:
        raise ValueError("njf_hip: grad must be a float32 GPU tensor; there is no CPU path")
    _note_device(grad, "grad")
    _launch("njf_scatter_footprint", load_library().njf_scatter_footprint, grad.data_ptr(), slices,
            grad.stride(0) if slices > 1 else 0, _int_ptr(foot_idx), _ptr(foot_w, "foot_w"), points, channels, out.shape[0],
            int(run_length), _ptr(out, "out"))


RESNET_BACKWARD_W_FLOATS = 21 * 8192
TRANSFORMER_BACKWARD_W_FLOATS = 13 * 8192    # NJF_TRANSFORMER_BACKWARD_CHUNKS
TRANSFORMER_BACKWARD_B_FLOATS = 3 * 192


def pack_transformer_backward(mats: torch.Tensor, biases: torch.Tensor, head_w: torch.Tensor, w_out: torch.Tensor,
                              b_out: torch.Tensor, precision: str = "f32") -> None:
    """Weights of njf_transformer_backward from the FOLDED head: mats [3,4,64,64] = (Mqk, Nov, W1', W2) per layer ([out, in]),
    biases [3,3,64] = (bqk, bo, b1'), head_w [3A,64] (include/njf_hip.h), packed for the chain's product form (``precision``:
    "f32" exact, or "f16x2")."""
    if precision not in BACKWARD_PRECISIONS:
        raise ValueError(f"njf_hip: backward precision must be one of {BACKWARD_PRECISIONS} (got {precision!r})")
    if tuple(mats.shape) != (3, 4, 64, 64) or tuple(biases.shape) != (3, 3, 64) or head_w.dim() != 2 or head_w.shape[1] != 64:
        raise ValueError("njf_hip: pack_transformer_backward shape mismatch")
    if w_out.numel() != TRANSFORMER_BACKWARD_W_FLOATS or b_out.numel() != TRANSFORMER_BACKWARD_B_FLOATS:
        raise ValueError("njf_hip: pack_transformer_backward output size mismatch")
    _launch("njf_pack_transformer_backward", load_library().njf_pack_transformer_backward, _ptr(mats.contiguous(), "mats"),
            _ptr(biases.contiguous(), "biases"), _ptr(head_w.contiguous(), "head_w"), head_w.shape[0], _ptr(w_out, "w_out"),
            _ptr(b_out, "b_out"), PRECISIONS[precision])


def transformer_backward(x: torch.Tensor, d_out: torch.Tensor, keys: int, w_backward: torch.Tensor, b_backward: torch.Tensor,
                         half_storage: bool = False, precision: str = "f32"):
    """The folded transformer head's data-gradient chain (include/njf_hip.h: njf_transformer_backward): x [4,P,64] (the residual
    stream the training forward dumped), d_out [P,3A] -> (wg_x [12,P,64], wg_dy [12,P,64], dx0 [P,64], column sums of the dY
    [12,64], unscale).  ``half_storage``: the pairs are fp16, the dY scaled by 2^k; ``unscale`` = 2^-k as a device scalar (else 1).
    ``precision``: the product form the weights were packed for ("f32" exact, "f16x2" split fp16 on d_out x 2^k)."""
    if precision not in BACKWARD_PRECISIONS:
        raise ValueError(f"njf_hip: backward precision must be one of {BACKWARD_PRECISIONS} (got {precision!r})")
    points = d_out.shape[0]
    if tuple(x.shape) != (4, points, 64) or w_backward.numel() != TRANSFORMER_BACKWARD_W_FLOATS \
            or b_backward.numel() != TRANSFORMER_BACKWARD_B_FLOATS:
        raise ValueError("njf_hip: transformer_backward shape mismatch")
    dev = d_out.device
    pair_dtype = torch.float16 if half_storage else torch.float32
    wg_x = torch.empty(12, points, 64, dtype=pair_dtype, device=dev)
    wg_dy = torch.empty(12, points, 64, dtype=pair_dtype, device=dev)
    dx0 = torch.empty(points, 64, dtype=torch.float32, device=dev)
    partial = torch.empty((points + 31) // 32, 12, 64, dtype=torch.float32, device=dev)
    d_out = d_out.contiguous()
    absmax = d_out.abs().amax().reshape(1) if (half_storage or precision != "f32") else None
    _launch("njf_transformer_backward", load_library().njf_transformer_backward, _ptr(x, "x"), _ptr(d_out, "d_out"), d_out.shape[1],
            int(keys), points, _ptr(w_backward, "w_backward"), _ptr(b_backward, "b_backward"), _ptr(wg_x, "wg_x", pair_dtype),
            _ptr(wg_dy, "wg_dy", pair_dtype), _ptr(dx0, "dx0"), _ptr(partial, "colsum_partial"), int(half_storage),
            _ptr(absmax, "d_out_absmax"), PRECISIONS[precision])
    unscale = power_of_two_unscale(absmax) if half_storage else None
    return wg_x, wg_dy, dx0, partial.sum(0), unscale


BACKWARD_PRECISIONS = ("f32", "f16x2")


def pack_resnetfc_backward(params: Dict[str, torch.Tensor], prefix: str, w_out: torch.Tensor, precision: str = "f32") -> None:
    """Transposed weights of one ResnetFC in the chunk order njf_resnetfc_backward streams them (include/njf_hip.h), packed for
    the chain's product form (``precision``: "f32" exact, or "f16x2")."""
    if precision not in BACKWARD_PRECISIONS:
        raise ValueError(f"njf_hip: backward precision must be one of {BACKWARD_PRECISIONS} (got {precision!r})")
    def p(name):
        return _ptr(params[prefix + name].detach().contiguous(), prefix + name)

    src = ResnetFcWeights()
    for i in range(5):
        src.fc0_w[i], src.fc1_w[i] = p(f"blocks.{i}.fc_0.weight"), p(f"blocks.{i}.fc_1.weight")
    src.lin_out_w = p("lin_out.weight")
    src.d_out = params[prefix + "lin_out.weight"].shape[0]
    _launch("njf_pack_resnetfc_backward", load_library().njf_pack_resnetfc_backward, C.byref(src), _ptr(w_out, "w_out"),
            PRECISIONS[precision])


def power_of_two_unscale(absmax: torch.Tensor) -> torch.Tensor:
    """2^-k for the k = 6 - exponent(max|d_out|) that njf_resnetfc_backward scales by (device-side, no host round trip)."""
    _, e = torch.frexp(absmax)                      # absmax = f * 2^e, f in [0.5, 1): the kernel's frexpf
    k = torch.clamp(6 - e, -120, 120)
    ok = (absmax > 0) & (absmax < 3.0e38)
    # 2^-k assembled from its exponent field (|k| <= 120: a normal number): torch.ldexp multiplies by a floating-point pow(2, -k),
    # which is not an exact power of two for every k on the device -- and the kernel's 2^k multiply is exact
    pow2 = ((127 - k).to(torch.int32) << 23).view(torch.float32)
    return torch.where(ok, pow2, torch.ones_like(absmax))


def resnetfc_backward_f16_storage(d_out: torch.Tensor, w_backward: torch.Tensor, mask: torch.Tensor, precision: str = "f32"):
    """The chain under the 16-bit training storage: -> (latent deltas [3,P,128] fp32 = slices 0, 2, 4, deltas16 [11,P,128] fp16 =
    deltas x 2^k, column sums [11,128] fp32, 2^-k as a device scalar)."""
    points = d_out.shape[0]
    if tuple(mask.shape) != (11, points, 4) or w_backward.numel() != RESNET_BACKWARD_W_FLOATS:
        raise ValueError("njf_hip: resnetfc_backward shape mismatch")
    if precision not in BACKWARD_PRECISIONS:
        raise ValueError(f"njf_hip: backward precision must be one of {BACKWARD_PRECISIONS} (got {precision!r})")
    dev = d_out.device
    latent = torch.empty(3, points, 128, dtype=torch.float32, device=dev)
    deltas16 = torch.empty(11, points, 128, dtype=torch.float16, device=dev)
    partial = torch.empty((points + 31) // 32, 11, 128, dtype=torch.float32, device=dev)
    d_out = d_out.contiguous()
    absmax = d_out.abs().amax().reshape(1)
    _launch("njf_resnetfc_backward", load_library().njf_resnetfc_backward, _ptr(d_out, "d_out"), d_out.shape[1], None,
            _ptr(w_backward, "w_backward"), points, _ptr(latent, "deltas"), _ptr(partial, "colsum_partial"), _int_ptr(mask),
            PRECISIONS[precision], _ptr(absmax, "d_out_absmax"), _ptr(deltas16, "deltas16", torch.float16))
    return latent, deltas16, partial.sum(0), power_of_two_unscale(absmax)


def resnetfc_backward(d_out: torch.Tensor, act: torch.Tensor, w_backward: torch.Tensor, want_colsum: bool = False,
                      mask: Optional[torch.Tensor] = None, precision: str = "f32"):
    """deltas [11,P,128] of one ResnetFC's backward pass (include/njf_hip.h: njf_resnetfc_backward): d_out [P,d_out],
    act [11,P,128] (dumped ReLU'd layer inputs), w_backward from pack_resnetfc_backward.  ``want_colsum``: also return
    the column sums [11,128] of every deltas slice (the bias gradients), reduced from the kernel's per-tile partials.
    ``mask`` [11,P,4] int32: the ReLU masks the same forward dumped (ABI v17) -- the chain then reads them instead of ``act``."""
    points = d_out.shape[0]
    if tuple(act.shape) != (11, points, 128) or w_backward.numel() != RESNET_BACKWARD_W_FLOATS:
        raise ValueError("njf_hip: resnetfc_backward shape mismatch")
    if mask is not None and tuple(mask.shape) != (11, points, 4):
        raise ValueError("njf_hip: resnetfc_backward mask must be [11, P, 4] int32")
    if precision not in BACKWARD_PRECISIONS:
        raise ValueError(f"njf_hip: backward precision must be one of {BACKWARD_PRECISIONS} (got {precision!r})")
    deltas = torch.empty_like(act)
    partial = torch.empty((points + 31) // 32, 11, 128, dtype=torch.float32, device=act.device) if want_colsum else None
    d_out = d_out.contiguous()
    # "f16x2": the chain runs on d_out scaled by a power of two taken from its largest entry (one reduction, no host round trip)
    absmax = d_out.abs().amax().reshape(1) if precision == "f16x2" else None
    _launch("njf_resnetfc_backward", load_library().njf_resnetfc_backward, _ptr(d_out, "d_out"), d_out.shape[1],
            _ptr(act, "act"), _ptr(w_backward, "w_backward"), points, _ptr(deltas, "deltas"), _ptr(partial, "colsum_partial"),
            _int_ptr(mask) if mask is not None else None, PRECISIONS[precision], _ptr(absmax, "d_out_absmax"), None)
    return (deltas, partial.sum(0)) if want_colsum else deltas


RELU_BACKWARD_ROWS = 512  # rows per workgroup of njf_relu_backward (one partial column-sum row each)


def relu_backward(upstream: torch.Tensor, act: torch.Tensor, residual: Optional[torch.Tensor] = None, want_colsum: bool = True):
    """(residual + upstream * [act > 0], its column sums) -- one layer step of the ResnetFC backward chain in one launch
    (include/njf_hip.h: njf_relu_backward).  All tensors [P,C] contiguous fp32 on the device."""
    points, channels = upstream.shape
    if act.shape != upstream.shape or (residual is not None and residual.shape != upstream.shape):
        raise ValueError("njf_hip: relu_backward shape mismatch")
    out = torch.empty_like(upstream)
    blocks = (points + RELU_BACKWARD_ROWS - 1) // RELU_BACKWARD_ROWS
    partial = torch.empty(blocks, channels, dtype=torch.float32, device=upstream.device) if want_colsum else None
    _launch("njf_relu_backward", load_library().njf_relu_backward, _ptr(upstream, "upstream"), _ptr(act, "act"), _ptr(residual, "residual"), points,
                                            channels, RELU_BACKWARD_ROWS, _ptr(out, "out"), _ptr(partial, "partial"))
    return out, (partial.sum(0) if want_colsum else None)


def bn_act(x: torch.Tensor, bn: "torch.nn.BatchNorm2d", skip: Optional[torch.Tensor] = None, relu: bool = True) -> torch.Tensor:
    """[relu](batch_norm_eval(x) [+ skip]) IN PLACE on x ([B,C,H,W] contiguous fp32, a convolution's fresh output): the epilogue of
    a convolution of the frozen encoder trunk as one launch (include/njf_hip.h: njf_bn_act).  ``bn``: an affine BatchNorm2d with
    running statistics, evaluated on them (eval mode)."""
    b, c, h, w = x.shape
    if skip is not None and (skip.shape != x.shape or not skip.is_contiguous() or skip.dtype != torch.float32):
        raise ValueError("njf_hip: bn_act skip must be a contiguous float32 tensor of x's shape")
    if not x.is_contiguous() or bn.running_mean is None or bn.weight is None or bn.weight.numel() != c:
        raise ValueError("njf_hip: bn_act needs a contiguous NCHW tensor and an affine BatchNorm2d with running statistics")
    _launch("njf_bn_act", load_library().njf_bn_act, _ptr(x, "x"), _ptr(bn.weight.detach(), "gamma"), _ptr(bn.bias.detach(), "beta"),
            _ptr(bn.running_mean, "running_mean"), _ptr(bn.running_var, "running_var"), float(bn.eps), _ptr(skip, "skip"), int(relu),
            b, c, h * w, _ptr(x, "out"))
    return x


def frame_partial_groups(total_rays: int) -> int:
    """Rows of NjfRenderOutputs.frame_partials for a launch of ``total_rays`` rays (one per workgroup)."""
    per = load_library().njf_rays_per_workgroup()
    return (total_rays + per - 1) // per


def reduce_frame_partials(partials: torch.Tensor, out4: torch.Tensor) -> None:
    """partials [groups,4] -> out4 [4] = (min_t, max_t, sum (rgb - trgt)^2, sum (flow - trgt)^2), fixed order."""
    _launch("njf_reduce_frame_partials", load_library().njf_reduce_frame_partials, _ptr(partials, "partials"),
            partials.shape[0], _ptr(out4, "out4"))


def assemble_frame(packets: torch.Tensor, batch: int, rays_per_batch: int, frame: torch.Tensor, scalars6: torch.Tensor,
                   rgb_scale: float = 0.0, flow_scale: float = 0.0) -> None:
    """packets [world, packet_floats] (all-gathered, include/njf_hip.h: njf_assemble_frame) -> frame [B,R,6] with the
    depth clipped to the global bounds, scalars6 = (min, max, S_rgb, S_flow, S_rgb * rgb_scale, S_flow * flow_scale)."""
    world, packet_floats = packets.shape
    if tuple(frame.shape) != (batch, rays_per_batch, 6) or scalars6.numel() != 6:
        raise ValueError("njf_hip: assemble_frame shape mismatch")
    _launch("njf_assemble_frame", load_library().njf_assemble_frame, _ptr(packets, "packets"), world, packet_floats, batch,
            rays_per_batch, float(rgb_scale), float(flow_scale), _ptr(frame, "frame"), _ptr(scalars6, "scalars6"))


def composite_backward(deltas, steps, sigma, color=None, g_weights=None, g_rgb=None, g_depth=None, want_color: bool = True):
    """(g_sigma [rays,S], g_color [rays,S,3] | None) of alpha compositing (njf_composite_backward): deltas / steps / sigma /
    g_weights [rays,S], color [rays,S,3], g_rgb [rays,3], g_depth [rays], contiguous fp32."""
    if deltas.dim() != 2:
        raise ValueError("njf_hip: composite_backward takes [rays, samples] fields")
    rays, samples = deltas.shape
    for name, t, shape in (("steps", steps, (rays, samples)), ("sigma", sigma, (rays, samples)), ("g_weights", g_weights, (rays, samples)),
                           ("color", color, (rays, samples, 3)), ("g_rgb", g_rgb, (rays, 3)), ("g_depth", g_depth, (rays,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"njf_hip: composite_backward: {name} has shape {tuple(t.shape)}, expected {shape}")
    g_sigma = torch.empty(rays, samples, dtype=torch.float32, device=deltas.device)
    g_color = torch.empty(rays, samples, 3, dtype=torch.float32, device=deltas.device) if (color is not None and want_color) else None
    _launch("njf_composite_backward", load_library().njf_composite_backward, _ptr(deltas, "deltas"), _ptr(steps, "steps"),
            _ptr(sigma, "sigma"), _ptr(color, "color"), _ptr(g_weights, "g_weights"), _ptr(g_rgb, "g_rgb"),
            _ptr(g_depth, "g_depth"), rays, samples, _ptr(g_sigma, "g_sigma"), _ptr(g_color, "g_color"))
    return g_sigma, g_color


def alpha_weights(deltas, densities, weights) -> None:
    samples = deltas.shape[-1]
    rays = deltas.numel() // samples
    _launch("njf_alpha_weights", load_library().njf_alpha_weights, _ptr(deltas), _ptr(densities), rays, samples, _ptr(weights))


def pdf_resample(weights, bins_in, u, s_out: int, anneal: float, bins_out) -> None:
    s_in = weights.shape[-1]
    rays = weights.numel() // s_in
    _launch("njf_pdf_resample", load_library().njf_pdf_resample, _ptr(weights), _ptr(bins_in), int(bins_in.dim() > 1), s_in, _ptr(u),
                                           int(u.dim() > 1), s_out, float(anneal), rays, _ptr(bins_out))
