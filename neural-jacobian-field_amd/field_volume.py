"""3-D Jacobian-field point clouds from a voxel grid, extracted on the device.

The reference colours point clouds of per-point Jacobians (``inference/jacobian_color_map.py:113-160``) but obtains them by
hand: a dense ``[B, N, 3]`` grid through ``Model.compute_density`` (model.py:416-456), then threshold / ``nonzero`` / gather.
Here the grid coordinates are generated inside the kernels, empty space is culled in stages -- context-view frustum, proposal
density, decoder density -- by an ORDERED stream compaction, and colour + Jacobian head run on the survivors only
(include/njf_hip.h: ``njf_field_points`` / ``njf_field_select`` / ``njf_field_forward``).

Definitions (fixed, so the result is checkable against the dense route):

* node ``(ix, iy, iz)`` of a grid has the linear index ``n = (ix*ny + iy)*nz + iz`` and the coordinate
  ``fma(i_c, step[c], origin[c])`` per component (one rounding, fp32);
* node ``n`` of batch element ``b`` has the global index ``b*N + n``, ``N = nx*ny*nz``, ``B*N < 2**31``;
* the extracted set is every node that passes the enabled predicates; it is returned in ASCENDING GLOBAL INDEX.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import geometry, hip
from .decoder import ActionDecoderFlowMlp, ActionDecoderJacobian, PixelEncoding, _cameras, _map_of
from .inference import jacobian_color_map as _cm


def _fma32(i: np.ndarray, step: np.float32, origin: np.float32) -> np.ndarray:
    """fp32 fma(i, step, origin): the product of an integer below 2**24 and an fp32 is exact in float64, so is its sum with an
    fp32 up to one float64 rounding far below half an fp32 ulp -- rounding that to fp32 is the fused result."""
    return (i.astype(np.float64) * np.float64(step) + np.float64(origin)).astype(np.float32)


@dataclass(frozen=True)
class FieldGrid:
    """A regular grid of ``dims = (nx, ny, nz)`` nodes: node ``(ix, iy, iz)`` sits at ``fma(i_c, step[c], origin[c])``."""

    origin: Tuple[float, float, float]
    step: Tuple[float, float, float]
    dims: Tuple[int, int, int]

    def __post_init__(self):
        if len(self.origin) != 3 or len(self.step) != 3 or len(self.dims) != 3:
            raise ValueError("FieldGrid: origin, step and dims have three components")
        if any(int(d) != d or d < 1 for d in self.dims):
            raise ValueError(f"FieldGrid: dims must be positive integers (got {self.dims})")
        object.__setattr__(self, "origin", tuple(float(np.float32(v)) for v in self.origin))
        object.__setattr__(self, "step", tuple(float(np.float32(v)) for v in self.step))
        object.__setattr__(self, "dims", tuple(int(d) for d in self.dims))
        if self.num_nodes >= 2 ** 31:
            raise ValueError("FieldGrid: nx*ny*nz must stay below 2**31")

    @classmethod
    def from_bounds(cls, lower: Sequence[float], upper: Sequence[float], resolution) -> "FieldGrid":
        """Nodes from ``lower`` to ``upper`` inclusive, ``resolution`` (an int or one per axis) per axis; an axis of one
        node sits at ``lower``."""
        res = (resolution,) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
        if len(res) != 3 or any(r < 1 for r in res):
            raise ValueError(f"FieldGrid.from_bounds: resolution must be >= 1 per axis (got {resolution})")
        step = tuple((float(u) - float(l)) / (r - 1) if r > 1 else 0.0 for l, u, r in zip(lower, upper, res))
        return cls(tuple(float(l) for l in lower), step, res)

    @property
    def num_nodes(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    def linear_index(self, ix, iy, iz):
        return (ix * self.dims[1] + iy) * self.dims[2] + iz

    def unravel(self, n):
        """linear (or, modulo ``num_nodes``, global) index -> (ix, iy, iz); ints, numpy arrays or tensors."""
        n = n % self.num_nodes
        yz = self.dims[1] * self.dims[2]
        return n // yz, (n % yz) // self.dims[2], n % self.dims[2]

    def points(self, indices: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
        """Node coordinates ``[count, 3]`` fp32: of all ``num_nodes`` nodes in linear order, or of ``indices`` (linear or global
        indices, any integer tensor).  On a GPU ``njf_field_points`` writes them (the very floats the extraction kernels
        evaluate); on the CPU the same fused multiply-add is evaluated with numpy."""
        if indices is not None and device is None:
            device = indices.device
        dev = torch.device("cpu" if device is None else device)
        if dev.type == "cuda":
            cg = self.c_grid()
            if indices is None:
                out = torch.empty(self.num_nodes, 3, dtype=torch.float32, device=dev)
                hip.field_points(cg, 1, None, None, self.num_nodes, out)
                return out
            idx = (indices.reshape(-1) % self.num_nodes).to(torch.int32).contiguous()
            out = torch.empty(idx.numel(), 3, dtype=torch.float32, device=dev)
            if idx.numel():
                hip.field_points(cg, 1, idx, None, idx.numel(), out)
            return out
        n = np.arange(self.num_nodes, dtype=np.int64) if indices is None else indices.reshape(-1).cpu().numpy().astype(np.int64)
        comps = self.unravel(n)
        xyz = np.stack([_fma32(i, np.float32(s), np.float32(o)) for i, s, o in zip(comps, self.step, self.origin)], axis=-1)
        return torch.from_numpy(xyz)

    def c_grid(self) -> "hip.FieldGrid":
        return hip.make_field_grid(self.origin, self.step, self.dims)


def _sensitivity_colors(owner: str, jacobian: Optional[torch.Tensor], rows: int, color_map, mode: int) -> torch.Tensor:
    """The joint-sensitivity colouring of the first ``rows`` Jacobians ``[n, A, 3]`` (point cloud and mesh alike)."""
    if jacobian is None:
        raise ValueError(f"{owner}.colors needs the Jacobians (extract with want_jacobian=True)")
    jac = jacobian[:rows]
    if isinstance(color_map, str):
        color_map = torch.tensor(_cm.JACOBIAN_COLORMAP[color_map], dtype=torch.float32).t()
    color_map = torch.as_tensor(color_map, dtype=torch.float32)
    if tuple(color_map.shape) != (3, jac.shape[1]):
        raise ValueError(f"{owner}.colors: color_map must be [3, {jac.shape[1]}] (got {tuple(color_map.shape)})")
    sens = _cm.compute_joint_sensitivity_point_cloud(jac)
    return _cm.visualize_joint_sensitivity_point_cloud(sens, color_map.to(jac.device), mode)


def _rgb8(owner: str, colors: Optional[torch.Tensor], default: Optional[torch.Tensor], n: int) -> np.ndarray:
    """``[n, 3]`` uint8 colours of a PLY: ``colors`` in [0, 1], else ``default`` (the colour head's output), else white."""
    rgb = default[:n] if colors is None and default is not None else colors
    rgb = np.ones((n, 3), dtype=np.float32) if rgb is None else rgb[:n].detach().float().cpu().numpy()
    if rgb.shape != (n, 3):
        raise ValueError(f"{owner}: colors must be [{n}, 3] (got {rgb.shape})")
    return np.rint(np.clip(rgb, 0.0, 1.0) * 255.0).astype(np.uint8)


@dataclass
class FieldPointCloud:
    """The extracted nodes in ascending global index.  Exactly sized (``count`` = number of rows) from an eager extraction;
    padded to ``max_points`` rows from a capture-safe one, where ``count`` (int32 device tensor ``[1]``) holds the TRUE number
    of survivors -- it may exceed the rows stored -- and rows from ``min(count, max_points)`` on are unspecified."""

    grid: FieldGrid
    index: torch.Tensor                 # [n] int32 global index b*N + n
    xyz: torch.Tensor                   # [n, 3]
    density: torch.Tensor               # [n]
    color: Optional[torch.Tensor]       # [n, 3]
    jacobian: Optional[torch.Tensor]    # [n, A, 3] action-major: compute_jacobian_at's rows reshaped
    count: torch.Tensor                 # [1] int32
    stage_counts: Tuple[torch.Tensor, ...] = ()   # survivors after each enabled selection stage, in pipeline order
    stage_names: Tuple[str, ...] = ()
    views: Optional[torch.Tensor] = None          # [n] uint8, fused extraction only: bit v = view v of the scene sees the node

    @property
    def batch_index(self) -> torch.Tensor:
        return torch.div(self.index, self.grid.num_nodes, rounding_mode="floor")

    def valid(self) -> int:
        """Rows that hold survivors (reads ``count``: a host synchronisation)."""
        return min(int(self.count.item()), self.index.shape[0])

    def colors(self, color_map, mode: int = 0) -> torch.Tensor:
        """``[n, 3]`` display colours in [0, 1]: ``compute_joint_sensitivity_point_cloud`` chained with
        ``visualize_joint_sensitivity_point_cloud`` (inference/jacobian_color_map.py) on the valid rows.  ``color_map``: a
        ``[3, A]`` tensor or the name of a table in ``JACOBIAN_COLORMAP`` (stored ``[A, 3]``)."""
        return _sensitivity_colors("FieldPointCloud", self.jacobian, self.valid(), color_map, mode)

    def save_ply(self, path, colors: Optional[torch.Tensor] = None) -> int:
        """Binary little-endian PLY of the valid rows: ``x y z`` float32, ``red green blue`` uint8, ``density`` float32.
        ``colors`` ``[n, 3]`` in [0, 1] (default: the colour head's output, white without one).  Returns the vertex count."""
        n = self.valid()
        rgb8 = _rgb8("save_ply", colors, self.color, n)
        vertex = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                                    ("density", "<f4")])
        xyz = self.xyz[:n].detach().cpu().numpy()
        vertex["x"], vertex["y"], vertex["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        vertex["red"], vertex["green"], vertex["blue"] = rgb8[:, 0], rgb8[:, 1], rgb8[:, 2]
        vertex["density"] = self.density[:n].detach().cpu().numpy()
        header = ("ply\nformat binary_little_endian 1.0\ncomment Jacobian-field point cloud\n"
                  f"element vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty float density\nend_header\n")
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(vertex.tobytes())
        return n


# ---- connected components -------------------------------------------------------------------------------
@dataclass
class FieldComponents:
    """Connected components of the inside nodes of a grid (``label_components``): ``labels[b, n]`` is the smallest global index
    of the node's component (-1 outside), ``sizes[b, n]`` its node count (0 outside), ``count`` the number of components,
    ``status`` 0 unless a loop of the device union-find passed its iteration cap (a defect: the eager entries raise on it)."""

    grid: FieldGrid
    labels: torch.Tensor    # [B, N] int32
    sizes: torch.Tensor     # [B, N] int32
    count: torch.Tensor     # [1] int32
    status: torch.Tensor    # [1] int32

    def keep(self, min_nodes: int = 1, largest_only: bool = False) -> torch.Tensor:
        """``[B, N]`` bool: the nodes of the components of at least ``min_nodes`` nodes; ``largest_only``: of those, per batch
        element, only the component of maximal size (ties go to the smallest label).  Integer torch ops on the tensors'
        device, no host read."""
        if isinstance(min_nodes, bool) or not isinstance(min_nodes, int) or min_nodes < 1:
            raise ValueError(f"FieldComponents.keep: min_nodes must be an integer >= 1 (got {min_nodes!r})")
        keep = self.sizes >= min_nodes                      # (an outside node has size 0)
        if largest_only:
            top = self.sizes.max(dim=1, keepdim=True).values
            none = torch.full_like(self.labels, torch.iinfo(torch.int32).max)
            first = torch.where((self.sizes == top) & (top > 0), self.labels, none).min(dim=1, keepdim=True).values
            keep = keep & (self.labels == first)
        return keep


def _check_component_arguments(name: str, connectivity, min_component_nodes=None) -> None:
    if isinstance(connectivity, bool) or connectivity not in hip.FIELD_COMPONENTS_CONNECTIVITIES:
        raise ValueError(f"{name}: connectivity must be 6 or 14 (got {connectivity!r})")
    if min_component_nodes is not None and (isinstance(min_component_nodes, bool) or not isinstance(min_component_nodes, int)
                                            or min_component_nodes < 1):
        raise ValueError(f"{name}: min_component_nodes must be an integer >= 1 (got {min_component_nodes!r})")


def _check_keys(name: str, keys, shape, like: torch.Tensor):
    if keys is None:
        return None
    if not torch.is_tensor(keys) or keys.dtype != torch.int32 or tuple(keys.shape) != tuple(shape):
        raise ValueError(f"{name}: keys must be int32 {tuple(shape)}")
    if keys.device != like.device:
        raise ValueError(f"{name}: keys must live on the device of the other tensors")
    return keys.contiguous()


def _raise_on_status(name: str, status: torch.Tensor) -> None:
    """The eager forms read the status word (a host synchronisation); nothing is read while a stream is being captured."""
    if status.is_cuda and torch.cuda.is_current_stream_capturing():
        return
    code = int(status.item())
    if code:
        raise RuntimeError(f"{name}: the device union-find passed an iteration cap (status {code}); its invariants are broken "
                           "and the labels are unspecified")


def _components(grid: FieldGrid, batch: int, connectivity: int, dev, **form) -> FieldComponents:
    """The four labelling launches on ``batch`` elements; ``form``: the dense or the list arguments of hip.field_components."""
    i32 = dict(dtype=torch.int32, device=dev)
    comp = FieldComponents(grid=grid, labels=torch.empty(batch, grid.num_nodes, **i32), sizes=torch.empty(batch, grid.num_nodes, **i32),
                           count=torch.empty(1, **i32), status=torch.empty(1, **i32))
    hip.field_components(grid.c_grid(), batch, connectivity, comp.labels, comp.sizes, comp.count, comp.status, **form)
    return comp


def label_components(grid: FieldGrid, values: torch.Tensor, threshold: float, *, valid: Optional[torch.Tensor] = None,
                     pixel_encoding: Optional[PixelEncoding] = None, connectivity: int = 6,
                     keys: Optional[torch.Tensor] = None) -> FieldComponents:
    """Connected components of any scalar on the grid, without the networks: ``values`` ``[B, N]`` fp32
    on the GPU; a node is inside iff it is valid -- ``valid`` ``[B, N]`` bool / uint8 and / or the frustum of the cameras of
    ``pixel_encoding``, the predicate of the selection and the mesher -- and ``values >= threshold`` (NaN is outside).  Inside
    nodes of one batch element are adjacent along the axes (``connectivity=6``) or along the edges of the Kuhn tetrahedra
    (``connectivity=14``, the mesh's own connectivity), without wrap at the grid faces; with ``keys`` ``[B, N]`` int32 only
    nodes of equal key are joined.  One host read (the status word) unless a stream is being captured."""
    if not torch.is_tensor(values) or values.dim() != 2 or values.dtype != torch.float32 or values.shape[1] != grid.num_nodes:
        raise ValueError(f"label_components: values must be fp32 [B, {grid.num_nodes}]")
    _check_component_arguments("label_components", connectivity)
    if not math.isfinite(float(threshold)):
        raise ValueError("label_components: the threshold must be finite")
    if values.shape[0] < 1 or values.shape[0] * grid.num_nodes >= 2 ** 31:
        raise ValueError("label_components: batch * nx*ny*nz must stay below 2**31")
    keys = _check_keys("label_components", keys, values.shape, values)
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8) or valid.shape != values.shape:
            raise ValueError(f"label_components: valid must be bool or uint8 {tuple(values.shape)}")
        if valid.device != values.device:
            raise ValueError("label_components: valid and values must live on the same device")
        valid = valid.contiguous()
    if pixel_encoding is not None and pixel_encoding.extrinsics.shape[0] != values.shape[0]:
        raise ValueError(f"label_components: {pixel_encoding.extrinsics.shape[0]} cameras for {values.shape[0]} rows of values")
    if values.device.type != "cuda":
        raise ValueError("label_components: values must live on the GPU; there is no CPU path")
    cams = None if pixel_encoding is None else _cameras(pixel_encoding, False, action_dim=None)
    comp = _components(grid, values.shape[0], connectivity, values.device, values=values.contiguous().reshape(-1),
                       threshold=float(threshold), valid=valid, cams=cams, keys=None if keys is None else keys.reshape(-1))
    _raise_on_status("label_components", comp.status)
    return comp


def _list_components(grid: FieldGrid, batch: int, index: torch.Tensor, count: Optional[torch.Tensor], capacity: int,
                     connectivity: int, keys: Optional[torch.Tensor] = None) -> FieldComponents:
    """The list form: the inside nodes are the first min(count, capacity) entries of the ascending ``index``."""
    return _components(grid, batch, connectivity, index.device, indices=index, list_count=count, capacity=capacity, keys=keys)


def cloud_components(cloud: FieldPointCloud, *, connectivity: int = 6, keys: Optional[torch.Tensor] = None,
                     batch: Optional[int] = None):
    """Components of the nodes of an extracted cloud, per row: ``(labels [n] int32, sizes [n] int32, count [1] int32)`` --
    the label is the smallest global index of the row's component among the cloud's nodes.  A padded cloud is labelled up to
    its ``count``, read on the device; rows past it get label -1 and size 0.  ``keys`` ``[n]`` int32 (e.g.
    ``dominant_joint(cloud.jacobian)``) joins only rows of equal key.  ``batch``: the number of batch elements (scenes) the
    cloud's grid was extracted for; None infers it from the largest index (one more host read)."""
    _check_component_arguments("cloud_components", connectivity)
    index = cloud.index
    n = index.shape[0]
    keys = _check_keys("cloud_components", keys, (n,), index)
    if index.device.type != "cuda":
        raise ValueError("cloud_components: the cloud must live on the GPU; there is no CPU path")
    nodes = cloud.grid.num_nodes
    rows = torch.arange(n, dtype=torch.int32, device=index.device) < cloud.count
    if batch is None:
        batch = int(torch.where(rows, index, torch.zeros_like(index)).max().item()) // nodes + 1 if n else 1
    if batch < 1 or batch * nodes >= 2 ** 31:
        raise ValueError("cloud_components: batch * nx*ny*nz must stay below 2**31")
    comp = _list_components(cloud.grid, batch, index.contiguous(), cloud.count, n, connectivity, keys)
    _raise_on_status("cloud_components", comp.status)
    at = index.clamp(0, batch * nodes - 1).long()
    minus = torch.full((n,), -1, dtype=torch.int32, device=index.device)
    return (torch.where(rows, comp.labels.reshape(-1)[at], minus), torch.where(rows, comp.sizes.reshape(-1)[at], minus + 1),
            comp.count)


def dominant_joint(jacobian: torch.Tensor) -> torch.Tensor:
    """``[n]`` int32: the action component whose Jacobian column moves the point most, ``argmax_a |J[a]|_2`` of ``jacobian``
    ``[n, A, 3]`` (compared through the squared norms ``x*x + y*y + z*z``, ties to the lowest a).  As ``keys`` of
    ``cloud_components`` it segments a cloud into the parts each joint moves most."""
    if not torch.is_tensor(jacobian) or jacobian.dim() != 3 or jacobian.shape[2] != 3 or jacobian.shape[1] < 1:
        raise ValueError("dominant_joint: jacobian must be [n, A, 3]")
    x, y, z = jacobian.unbind(dim=2)
    return torch.argmax(x * x + y * y + z * z, dim=1).to(torch.int32)


def _component_flags(grid: FieldGrid, batch: int, index: torch.Tensor, count: Optional[torch.Tensor], extent: int,
                     connectivity: int, min_nodes: Optional[int], largest_only: bool, eager: bool):
    """fp32 0 / 1 per list entry: the entry's component (among the list's nodes) survives the filter; and the status word."""
    comp = _list_components(grid, batch, index, count, extent, connectivity)
    if eager:
        _raise_on_status("extract_field", comp.status)
    keep = comp.keep(1 if min_nodes is None else min_nodes, largest_only).reshape(-1)
    # (rows past the device count of a capacity form hold no index: clamped, and the selection never reads their flag)
    return keep[index[:extent].clamp(0, batch * grid.num_nodes - 1).long()].to(torch.float32), comp.status


# ---- rigid twists per part and command channel -----------------------------------------------------------
@dataclass
class FieldTwists:
    """The rigid field ``J_a(x) = velocity[p, a] + omega[p, a] x (x - centroid[p])`` fitted to the Jacobians of every part p and
    command channel a (``fit_twists``; include/njf_hip.h: njf_field_twists): six numbers, a screw axis, per part and channel.
    ``labels[p]`` is the part's label (-1: an unused slot, all zeros), ``count`` the TRUE number of parts (it may exceed the K
    slots), ``nodes`` the rows of the part, ``status`` 0 or bits: 1 = no row of positive weight (the slot is zero), 2 =
    translation-only (one node or collinear nodes: ``omega`` is not determined and set to 0).  ``energy = sum w |J|^2`` and
    ``residual = sum w |J - model|^2`` per part and channel; ``Q`` (xx, xy, xz, yy, yz, zz), ``P``, ``L`` are the raw weighted
    sums of the fit; ``row_residual[i] = sum_a |J_a - model|^2`` (unweighted, 0 for rows of no fitted part)."""

    labels: torch.Tensor         # [K] int32
    count: torch.Tensor          # [1] int32
    nodes: torch.Tensor          # [K] int32
    status: torch.Tensor         # [K] int32
    weight: torch.Tensor         # [K] float64
    centroid: torch.Tensor       # [K, 3] float64
    omega: torch.Tensor          # [K, A, 3] float64
    velocity: torch.Tensor       # [K, A, 3] float64: at the centroid
    energy: torch.Tensor         # [K, A] float64
    residual: torch.Tensor       # [K, A] float64
    Q: torch.Tensor              # [K, 6] float64
    P: torch.Tensor              # [K, A, 3] float64
    L: torch.Tensor              # [K, A, 3] float64
    row_residual: torch.Tensor   # [n] fp32

    def rigidity(self) -> torch.Tensor:
        """``[K, A]``: the share of the field the rigid model explains, ``1 - residual / energy`` (1 where the energy is 0)."""
        zero = self.energy == 0
        return torch.where(zero, 1.0, 1.0 - self.residual / torch.where(zero, 1.0, self.energy))

    def screw(self, eps: float = 1e-9):
        """``(direction [K, A, 3], point [K, A, 3], pitch [K, A])`` of the screw axis of every twist: the unit direction of
        ``omega``, the point ``c + omega x v / |omega|^2`` of the axis nearest the centroid and the pitch ``omega . v /
        |omega|^2`` (translation along the axis per radian).  Where ``|omega| * extent <= eps * |v|`` (prismatic; extent =
        ``sqrt(tr Q / W)``, the part's RMS radius) the direction is that of ``v``, the point the centroid and the pitch inf; a
        zero twist has direction 0."""
        w, v = self.omega, self.velocity
        wn, vn = torch.linalg.vector_norm(w, dim=-1), torch.linalg.vector_norm(v, dim=-1)
        safe = torch.where(self.weight > 0, self.weight, torch.ones_like(self.weight))
        extent = torch.sqrt((self.Q[:, 0] + self.Q[:, 3] + self.Q[:, 5]) / safe)[:, None]
        prismatic = wn * extent <= eps * vn
        w2 = torch.where(prismatic, torch.ones_like(wn), wn * wn)
        centre = self.centroid[:, None, :].expand_as(w)
        unit_v = v / torch.where(vn > 0, vn, torch.ones_like(vn))[..., None]
        direction = torch.where(prismatic[..., None], unit_v, w / torch.sqrt(w2)[..., None])
        point = torch.where(prismatic[..., None], centre, centre + torch.linalg.cross(w, v, dim=-1) / w2[..., None])
        pitch = torch.where(prismatic, torch.full_like(wn, math.inf), (w * v).sum(-1) / w2)
        return direction, point, pitch

    def jacobian_at(self, xyz: torch.Tensor, slot: int) -> torch.Tensor:
        """The model's Jacobians ``[m, A, 3]`` (float64) of part ``slot`` at the points ``xyz`` ``[m, 3]``."""
        r = xyz.to(self.centroid.dtype) - self.centroid[slot]
        return self.velocity[slot][None] + torch.linalg.cross(self.omega[slot][None].expand(r.shape[0], -1, 3),
                                                               r[:, None, :].expand(-1, self.omega.shape[1], 3), dim=-1)


def _check_labels(name: str, labels, n: int, optional: bool = False) -> None:
    if optional and labels is None:
        return
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or tuple(labels.shape) != (n,):
        raise ValueError(f"{name}: labels must be int32 [{n}]")


def _posed_points(name: str, points, layout: str):
    """``points`` fp32 ``[n, 3]`` or ``[<layout>, n, 3]`` as the 3-D tensor, and its ``(Mq, n)``."""
    if not torch.is_tensor(points) or points.dtype != torch.float32 or points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise ValueError(f"{name}: points must be fp32 [n, 3] or [{layout}, n, 3]")
    points = points if points.dim() == 3 else points[None]
    return points, tuple(points.shape[:2])


def _one_int32(name: str, what: str, t, like: torch.Tensor):
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.numel() != 1:
        raise ValueError(f"{name}: {what} must be one int32 (a device tensor)")
    if t.device != like.device:
        raise ValueError(f"{name}: {what} must live on the device of the other tensors")
    return t


def fit_twists(xyz: torch.Tensor, jacobian: torch.Tensor, labels: torch.Tensor, parts: torch.Tensor, *,
               parts_count: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
               weights: Optional[torch.Tensor] = None) -> FieldTwists:
    """Least-squares rigid twist of every part and command channel: rows ``xyz`` ``[n, 3]`` and
    ``jacobian`` ``[n, A, 3]`` fp32 -- of a cloud, or the vertices of a mesh --, ``labels`` ``[n]`` int32 (negative: no part),
    ``parts`` ``[K]`` int32, ascending, distinct and non-negative, K <= 256, of which the first ``min(parts_count, K)`` are
    fitted (``parts_count``: int32 device tensor, the true number of parts; None = K); rows from ``count`` (int32 device
    tensor; None = n) on are never read; ``weights`` ``[n]`` fp32 (NaN and negatives count as 0; None = 1).  All sums are in
    float64 in a fixed order, without atomics: two calls give equal bytes, and nothing is read on the host."""
    name = "fit_twists"
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float32:
        raise ValueError(f"{name}: xyz must be fp32 [n, 3]")
    n = xyz.shape[0]
    if (not torch.is_tensor(jacobian) or jacobian.dim() != 3 or jacobian.dtype != torch.float32 or jacobian.shape[0] != n
            or jacobian.shape[2] != 3 or jacobian.shape[1] < 1):
        raise ValueError(f"{name}: jacobian must be fp32 [{n}, A, 3]")
    a_dim = jacobian.shape[1]
    if a_dim > hip.MAX_ACTION_DIM:
        raise ValueError(f"{name}: at most {hip.MAX_ACTION_DIM} command channels (got {a_dim})")
    _check_labels(name, labels, n)
    if not torch.is_tensor(parts) or parts.dtype != torch.int32 or parts.dim() != 1:
        raise ValueError(f"{name}: parts must be int32 [K]")
    k = parts.shape[0]
    if not 1 <= k <= hip.FIELD_TWISTS_MAX_PARTS:
        raise ValueError(f"{name}: parts must hold 1 to {hip.FIELD_TWISTS_MAX_PARTS} labels (got {k})")
    if weights is not None and (not torch.is_tensor(weights) or weights.dtype != torch.float32 or tuple(weights.shape) != (n,)):
        raise ValueError(f"{name}: weights must be fp32 [{n}]")
    for what, t in (("jacobian", jacobian), ("labels", labels), ("parts", parts), ("weights", weights)):
        if t is not None and t.device != xyz.device:
            raise ValueError(f"{name}: {what} must live on the device of xyz")
    count = _one_int32(name, "count", count, xyz)
    parts_count = _one_int32(name, "parts_count", parts_count, xyz)
    if hip.field_twists_workspace(n, k, a_dim) >= 2 ** 31:
        raise ValueError(f"{name}: {n} rows with {k} parts overflow the partial sums")
    if xyz.device.type != "cuda":
        raise ValueError(f"{name}: the rows must live on the GPU; there is no CPU path")
    dev = xyz.device
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    tw = FieldTwists(labels=torch.empty(k, **i32), count=torch.empty(1, **i32), nodes=torch.empty(k, **i32),
                     status=torch.empty(k, **i32), weight=torch.empty(k, **f64), centroid=torch.empty(k, 3, **f64),
                     omega=torch.empty(k, a_dim, 3, **f64), velocity=torch.empty(k, a_dim, 3, **f64),
                     energy=torch.empty(k, a_dim, **f64), residual=torch.empty(k, a_dim, **f64), Q=torch.empty(k, 6, **f64),
                     P=torch.empty(k, a_dim, 3, **f64), L=torch.empty(k, a_dim, 3, **f64),
                     row_residual=torch.empty(n, dtype=torch.float32, device=dev))
    out = dict(labels=tw.labels, count=tw.count, nodes=tw.nodes, status=tw.status, weight=tw.weight, centroid=tw.centroid,
               omega=tw.omega, velocity=tw.velocity, energy=tw.energy, residual=tw.residual, q=tw.Q, p=tw.P, l=tw.L,
               row_residual=tw.row_residual)
    hip.field_twists(xyz.contiguous(), jacobian.contiguous(), labels.contiguous(), parts.contiguous(), out,
                     weights=None if weights is None else weights.contiguous(), count=count, parts_count=parts_count)
    return tw


def cloud_twists(cloud: FieldPointCloud, *, labels: Optional[torch.Tensor] = None, sizes: Optional[torch.Tensor] = None,
                 connectivity: int = 6, keys: Optional[torch.Tensor] = None, min_nodes: int = 1, max_parts: int = 32,
                 weights="density", batch: Optional[int] = None) -> FieldTwists:
    """``fit_twists`` on the parts of an extracted cloud.  ``labels`` / ``sizes`` ``[n]`` int32: the per-row result of
    ``cloud_components`` (both or neither; without them it runs here with ``connectivity``, ``keys`` -- e.g.
    ``dominant_joint(cloud.jacobian)`` -- and ``batch``).  The parts are the components of at least ``min_nodes`` nodes, in
    ascending label; the first ``max_parts`` (1..256) of them are fitted and ``count`` holds their true number.  The part
    list is built on the device: the root rows (``labels == cloud.index``, ``sizes >= min_nodes``, row < ``cloud.count``) pass
    through the ordered selection on ``cloud.index``, so nothing is read on the host (given ``batch``, or the labels).
    ``weights``: ``"density"`` (the cloud's), None (uniform) or an fp32 ``[n]`` tensor."""
    name = "cloud_twists"
    if cloud.jacobian is None:
        raise ValueError(f"{name} needs the Jacobians (extract with want_jacobian=True)")
    if isinstance(max_parts, bool) or not isinstance(max_parts, int) or not 1 <= max_parts <= hip.FIELD_TWISTS_MAX_PARTS:
        raise ValueError(f"{name}: max_parts must be an integer in [1, {hip.FIELD_TWISTS_MAX_PARTS}] (got {max_parts!r})")
    if isinstance(min_nodes, bool) or not isinstance(min_nodes, int) or min_nodes < 1:
        raise ValueError(f"{name}: min_nodes must be an integer >= 1 (got {min_nodes!r})")
    _check_component_arguments(name, connectivity)
    index = cloud.index
    n = index.shape[0]
    if cloud.jacobian.shape[1] > hip.MAX_ACTION_DIM:
        raise ValueError(f"{name}: at most {hip.MAX_ACTION_DIM} command channels (got {cloud.jacobian.shape[1]})")
    if (labels is None) != (sizes is None):
        raise ValueError(f"{name}: labels and sizes come together (the per-row result of cloud_components)")
    for what, t in (("labels", labels), ("sizes", sizes)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != (n,) or t.device != index.device):
            raise ValueError(f"{name}: {what} must be int32 [{n}] on the cloud's device")
    if isinstance(weights, str):
        if weights != "density":
            raise ValueError(f"{name}: weights must be \"density\", None or a tensor (got {weights!r})")
        weights = cloud.density
    if weights is not None and (not torch.is_tensor(weights) or weights.dtype != torch.float32 or tuple(weights.shape) != (n,)
                                or weights.device != index.device):
        raise ValueError(f"{name}: weights must be fp32 [{n}] on the cloud's device")
    if index.device.type != "cuda":
        raise ValueError(f"{name}: the cloud must live on the GPU; there is no CPU path")
    if labels is None:
        labels, sizes, _ = cloud_components(cloud, connectivity=connectivity, keys=keys, batch=batch)
    dev = index.device
    parts = torch.full((max_parts,), -1, dtype=torch.int32, device=dev)
    parts_count = torch.zeros(1, dtype=torch.int32, device=dev)
    if n > 0:
        rows = torch.arange(n, dtype=torch.int32, device=dev) < cloud.count
        roots = ((labels == index) & (sizes >= min_nodes) & rows).to(torch.float32)
        nodes = cloud.grid.num_nodes
        # (the selection needs only an upper bound of the batch: it clamps the indices it copies into the grid's range)
        span = (2 ** 31 - 1) // nodes if batch is None else batch
        hip.field_select(cloud.grid.c_grid(), span, n, parts, parts_count, values=roots, threshold=0.5, indices=index.contiguous(),
                         count=cloud.count)
    return fit_twists(cloud.xyz, cloud.jacobian, labels, parts, parts_count=parts_count, count=cloud.count, weights=weights)


# ---- joints between parts: grid contacts and relative twists ---------------------------------------------
@dataclass
class FieldJoints:
    """The pairs of parts that touch on the grid (``part_joints``; include/njf_hip.h: njf_field_joints), in ascending
    ``(part_a, part_b)`` -- slots of ``twists``, ``part_a < part_b``; ``labels`` are the twists' part labels, so joint j joins
    the parts ``labels[part_a[j]]`` and ``labels[part_b[j]]``.  ``contacts`` counts the adjacent node pairs, ``anchor`` is their
    mean midpoint, ``omega`` / ``velocity`` the twist of part_b relative to part_a per command channel, the velocity taken AT
    the anchor: the relative twist is the joint, its screw axis the hinge, and the velocity at the contact says how far the
    pair is from a revolute one.  ``status`` = the two parts' twist status bits or-ed.  ``count`` is the TRUE number of joints
    (it may exceed the J rows); unused rows hold -1 in ``part_a`` / ``part_b`` and zeros elsewhere."""

    grid: FieldGrid
    labels: torch.Tensor      # [K] int32: the twists' part labels
    part_a: torch.Tensor      # [J] int32
    part_b: torch.Tensor      # [J] int32
    contacts: torch.Tensor    # [J] int64
    status: torch.Tensor      # [J] int32
    count: torch.Tensor       # [1] int32
    anchor: torch.Tensor      # [J, 3] float64
    omega: torch.Tensor       # [J, A, 3] float64
    velocity: torch.Tensor    # [J, A, 3] float64: at the anchor
    twists: Optional[FieldTwists] = None   # the parts' own twists (``parents`` takes its default root from them)

    def _length(self, length) -> float:
        return float(max(abs(s) for s in self.grid.step)) if length is None else float(length)

    def screw(self, eps: float = 1e-9):
        """``(direction [J, A, 3], point [J, A, 3], pitch [J, A])`` of the screw axis of every relative twist: the definition
        of ``FieldTwists.screw`` with the anchor in place of the centroid -- the unit direction of ``omega``, the point ``anchor
        + omega x v / |omega|^2`` of the axis nearest the anchor, the pitch ``omega . v / |omega|^2``.  A contact has no RMS
        radius, so the prismatic test ``|omega| * extent <= eps * |v|`` takes the largest grid step as ``extent``; there the
        direction is that of ``v``, the point the anchor and the pitch inf; a zero twist has direction 0."""
        w, v = self.omega, self.velocity
        wn, vn = torch.linalg.vector_norm(w, dim=-1), torch.linalg.vector_norm(v, dim=-1)
        prismatic = wn * self._length(None) <= eps * vn
        w2 = torch.where(prismatic, torch.ones_like(wn), wn * wn)
        centre = self.anchor[:, None, :].expand_as(w)
        unit_v = v / torch.where(vn > 0, vn, torch.ones_like(vn))[..., None]
        direction = torch.where(prismatic[..., None], unit_v, w / torch.sqrt(w2)[..., None])
        point = torch.where(prismatic[..., None], centre, centre + torch.linalg.cross(w, v, dim=-1) / w2[..., None])
        pitch = torch.where(prismatic, torch.full_like(wn, math.inf), (w * v).sum(-1) / w2)
        return direction, point, pitch

    def drive(self, length: Optional[float] = None) -> torch.Tensor:
        """``[J]`` int64: the command channel that moves the pair most, ``argmax_a (|omega_rel|^2 * length^2 + |v_rel|^2)``, ties
        to the lowest a (0 for an unused row).  ``length`` turns a rotation into a speed; default: the largest grid step."""
        length = self._length(length)
        w2, v2 = (self.omega * self.omega).sum(-1), (self.velocity * self.velocity).sum(-1)
        return torch.argmax(w2 * (length * length) + v2, dim=1)

    def parents(self, root: Optional[int] = None):
        """``(parent [K], joint_of [K])``, int64 CPU tensors: the kinematic tree.  The stored joints form a graph on the slots;
        its MAXIMUM SPANNING FOREST by ``contacts`` (ties to the smaller ``(part_a, part_b)``) is oriented away from a root per
        body.  ``parent[p]`` is the slot p hangs on and ``joint_of[p]`` the row of the joint between them; both are -1 for a
        root and for an unused slot.  ``root``: a slot; its body hangs on it.  Every other body -- every body with ``root=None``
        -- hangs on its slot of smallest ``sum_a energy / weight`` among those of twist status 0, the base (ties, or no such
        slot, or no ``twists``: the smallest slot).  Host-side numpy on ONE host read of the few numbers it needs."""
        k, rows = self.labels.shape[0], self.part_a.shape[0]
        if root is not None and (isinstance(root, bool) or not isinstance(root, int) or not 0 <= root < k):
            raise ValueError(f"FieldJoints.parents: root must be a slot in [0, {k}) (got {root!r})")
        f64 = dict(dtype=torch.float64, device=self.part_a.device)
        mobility = torch.zeros(k, **f64)
        if self.twists is not None:
            tw = self.twists
            base = (tw.status == 0) & (tw.weight > 0)
            mobility = torch.where(base, tw.energy.sum(1) / torch.where(base, tw.weight, torch.ones_like(tw.weight)),
                                   torch.full_like(tw.weight, math.inf)).to(**f64)
        packed = torch.cat([self.count.to(**f64), self.labels.to(**f64), mobility, self.part_a.to(**f64), self.part_b.to(**f64),
                            self.contacts.to(**f64)]).cpu().numpy()        # the one host read
        stored = min(max(int(packed[0]), 0), rows)
        labels, mobility = packed[1:1 + k], packed[1 + k:1 + 2 * k]
        lo, hi, contacts = (packed[1 + 2 * k + i * rows:1 + 2 * k + i * rows + stored].astype(np.int64) for i in range(3))
        if root is not None and labels[root] < 0:
            raise ValueError(f"FieldJoints.parents: slot {root} is unused")
        group = np.arange(k)

        def find(x):
            while group[x] != x:
                group[x] = group[group[x]]
                x = group[x]
            return x

        links = [[] for _ in range(k)]
        for j in sorted(range(stored), key=lambda j: (-contacts[j], lo[j], hi[j])):
            a, b = find(lo[j]), find(hi[j])
            if a != b:
                group[max(a, b)] = min(a, b)
                links[lo[j]].append((int(hi[j]), j))
                links[hi[j]].append((int(lo[j]), j))
        parent, joint_of = np.full(k, -1, dtype=np.int64), np.full(k, -1, dtype=np.int64)
        bodies = {}
        for p in range(k):
            if labels[p] >= 0:
                bodies.setdefault(find(p), []).append(p)
        for members in bodies.values():
            start = root if root in members else min(members, key=lambda p: (mobility[p], p))
            seen, queue = {start}, [start]
            while queue:
                p = queue.pop()
                for q, j in links[p]:
                    if q not in seen:
                        seen.add(q)
                        parent[q], joint_of[q] = p, j
                        queue.append(q)
        return torch.from_numpy(parent), torch.from_numpy(joint_of)

    def tree(self, root: Optional[int] = None):
        """``parents(root)`` as the two int32 tensors on the joints' device that ``part_poses`` / ``cloud_pose`` take."""
        parent, joint_of = self.parents(root)
        return parent.to(device=self.part_a.device, dtype=torch.int32), joint_of.to(device=self.part_a.device, dtype=torch.int32)


def part_joints(grid: FieldGrid, index: torch.Tensor, labels: torch.Tensor, twists: FieldTwists, *, batch: int,
                count: Optional[torch.Tensor] = None, connectivity: int = 6, min_contacts: int = 1,
                max_joints: int = 256) -> FieldJoints:
    """The joints between the parts of a labelled list of grid nodes: ``index`` ``[n]`` int32, the
    ascending global indices of the rows on ``grid`` x ``batch`` (rows from ``count`` -- int32 device tensor; None = n -- on are
    never read, an index outside the grid is dropped), ``labels`` ``[n]`` int32, the per-row result of ``cloud_components``
    (negative: no part), and ``twists``, the ``FieldTwists`` fitted to those labels, whose part list defines the slots.  Two
    slots are in contact where a node of one has a node of the other as its neighbour along the axes (``connectivity=6``) or
    the edges of the Kuhn tetrahedra (``14``), inside the grid and one batch element; pairs with at least ``min_contacts``
    contacts are listed in ascending ``(part_a, part_b)``, the first ``max_joints`` (1..4096) stored.  Integer atomics and
    per-joint double arithmetic only: two calls give equal bytes, and nothing is read on the host."""
    return _joints("part_joints", grid, index, labels, twists, batch, count, connectivity, min_contacts, max_joints)


def _joints(name: str, grid: FieldGrid, index, labels, twists, batch, count, connectivity, min_contacts, max_joints,
            infer_batch: bool = False) -> FieldJoints:
    """The argument checks (under the caller's ``name``) and the launches of part_joints / cloud_joints.  ``infer_batch``: a
    ``batch`` of None is read from the largest index once every check has passed."""
    _check_component_arguments(name, connectivity)
    for what, v, top in (("min_contacts", min_contacts, 2 ** 31 - 1), ("max_joints", max_joints, hip.FIELD_JOINTS_MAX)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
            raise ValueError(f"{name}: {what} must be an integer in [1, {top}] (got {v!r})")
    if not (batch is None and infer_batch) and (isinstance(batch, bool) or not isinstance(batch, int) or batch < 1
                                                or batch * grid.num_nodes >= 2 ** 31):
        raise ValueError(f"{name}: batch must be an integer >= 1 with batch * nx*ny*nz below 2**31 (got {batch!r})")
    if not torch.is_tensor(index) or index.dtype != torch.int32 or index.dim() != 1:
        raise ValueError(f"{name}: index must be int32 [n]")
    n = index.shape[0]
    _check_labels(name, labels, n)
    if not isinstance(twists, FieldTwists):
        raise ValueError(f"{name}: twists must be a FieldTwists")
    parts = twists.labels
    if not torch.is_tensor(parts) or parts.dtype != torch.int32 or parts.dim() != 1:
        raise ValueError(f"{name}: twists.labels must be int32 [K]")
    k = parts.shape[0]
    if not 1 <= k <= hip.FIELD_TWISTS_MAX_PARTS:
        raise ValueError(f"{name}: the twists must hold 1 to {hip.FIELD_TWISTS_MAX_PARTS} parts (got {k})")
    omega = twists.omega
    if not torch.is_tensor(omega) or omega.dtype != torch.float64 or omega.dim() != 3 or omega.shape[0] != k or omega.shape[2] != 3:
        raise ValueError(f"{name}: twists.omega must be float64 [{k}, A, 3]")
    a_dim = omega.shape[1]
    if not 1 <= a_dim <= hip.MAX_ACTION_DIM:
        raise ValueError(f"{name}: 1 to {hip.MAX_ACTION_DIM} command channels (got {a_dim})")
    for what, t, dtype, shape in (("velocity", twists.velocity, torch.float64, (k, a_dim, 3)),
                                  ("centroid", twists.centroid, torch.float64, (k, 3)), ("status", twists.status, torch.int32, (k,))):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f"{name}: twists.{what} must be {str(dtype).replace('torch.', '')} {list(shape)}")
    count = _one_int32(name, "count", count, index)
    parts_count = _one_int32(name, "twists.count", twists.count, index)
    for what, t in (("labels", labels), ("twists.labels", parts), ("twists.omega", omega), ("twists.velocity", twists.velocity),
                    ("twists.centroid", twists.centroid), ("twists.status", twists.status)):
        if t.device != index.device:
            raise ValueError(f"{name}: {what} must live on the device of index")
    if index.device.type != "cuda":
        raise ValueError(f"{name}: the rows must live on the GPU; there is no CPU path")
    dev = index.device
    if batch is None:
        rows = torch.arange(n, dtype=torch.int32, device=dev) < (n if count is None else count)
        batch = int(torch.where(rows, index, torch.zeros_like(index)).max().item()) // grid.num_nodes + 1 if n else 1
        if batch * grid.num_nodes >= 2 ** 31:
            raise ValueError(f"{name}: batch * nx*ny*nz must stay below 2**31")
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    j = max_joints
    joints = FieldJoints(grid=grid, labels=parts, part_a=torch.empty(j, **i32), part_b=torch.empty(j, **i32),
                         contacts=torch.empty(j, dtype=torch.int64, device=dev), status=torch.empty(j, **i32),
                         count=torch.empty(1, **i32), anchor=torch.empty(j, 3, **f64), omega=torch.empty(j, a_dim, 3, **f64),
                         velocity=torch.empty(j, a_dim, 3, **f64), twists=twists)
    out = dict(part_a=joints.part_a, part_b=joints.part_b, contacts=joints.contacts, status=joints.status, count=joints.count,
               anchor=joints.anchor, omega=joints.omega, velocity=joints.velocity)
    hip.field_joints(grid.c_grid(), batch, index.contiguous(), labels.contiguous(), parts.contiguous(), twists.status.contiguous(),
                     twists.centroid.contiguous(), omega.contiguous(), twists.velocity.contiguous(), out, count=count,
                     parts_count=parts_count, connectivity=connectivity, min_contacts=min_contacts)
    return joints


def cloud_joints(cloud: FieldPointCloud, labels: torch.Tensor, twists: FieldTwists, *, batch: Optional[int] = None,
                 connectivity: int = 6, min_contacts: int = 1, max_joints: int = 256) -> FieldJoints:
    """``part_joints`` on an extracted cloud: its grid, ``cloud.index`` and ``cloud.count``, with ``labels`` ``[n]`` int32 (the
    per-row result of ``cloud_components``) and the ``twists`` of ``cloud_twists(cloud, labels=, sizes=)``.  ``batch``: the
    number of batch elements (scenes) the cloud's grid was extracted for; None infers it from the largest index, as
    ``cloud_components`` does (one host read); given ``batch``, nothing is read."""
    return _joints("cloud_joints", cloud.grid, cloud.index, labels, twists, batch, cloud.count, connectivity, min_contacts,
                   max_joints, infer_batch=True)


# ---- posing the parts under a command: twist exponentials along the tree ---------------------------------
@dataclass
class FieldPose:
    """The rigid motion of every part under every command (``part_poses``; include/njf_hip.h: njf_field_pose): ``x -> rotation[m,
    p] x + translation[m, p]`` takes a point of part ``labels[p]`` from the present configuration to the one under ``commands[m]``
    -- the product of the exponentials of the joint twists along the part's chain to the root, or, without a tree, the
    exponential of the part's own twist about its centroid.  ``status`` 0 or bits: 1 = the slot is unused or its twist is empty
    (its own motion is the identity), 2 = the slot hangs on a bad link, a cycle or a parent outside the list (its pose is the
    identity).  ``depth`` counts the links above the slot.  ``count`` is the twists' TRUE number of parts."""

    labels: torch.Tensor        # [K] int32: the twists' part labels
    count: torch.Tensor         # [1] int32
    rotation: torch.Tensor      # [M, K, 3, 3] float64
    translation: torch.Tensor   # [M, K, 3] float64
    status: torch.Tensor        # [K] int32
    depth: torch.Tensor         # [K] int32
    commands: torch.Tensor      # [M, A] fp32

    def matrix(self) -> torch.Tensor:
        """``[M, K, 4, 4]`` float64: the homogeneous matrices."""
        m, k = self.rotation.shape[:2]
        out = torch.zeros(m, k, 4, 4, dtype=self.rotation.dtype, device=self.rotation.device)
        out[..., :3, :3] = self.rotation
        out[..., :3, 3] = self.translation
        out[..., 3, 3] = 1.0
        return out

    def apply(self, xyz: torch.Tensor, labels: torch.Tensor, *, count: Optional[torch.Tensor] = None,
              jacobian: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``[M, n, 3]`` fp32: the points ``xyz`` ``[n, 3]`` (fp32) with part labels ``labels`` ``[n]`` (int32; the rows of a
        cloud, mesh vertices with the label of their owner node, ...) under every command.  A row whose label is a part of
        status 0 moves with the part, in double, rounded once.  Every other row below ``count`` (int32 device tensor; None = n)
        takes the field's own first-order step ``x + sum_a u_a J_a`` when ``jacobian`` ``[n, A, 3]`` (fp32) is given, and stays
        where it is otherwise.  Rows from ``count`` on are not written (the result is allocated, not cleared)."""
        name = "FieldPose.apply"
        m, a_dim = self.commands.shape
        n = _check_points(name, xyz, labels, jacobian, a_dim)
        count = _one_int32(name, "count", count, xyz)
        for what, t in (("labels", labels), ("jacobian", jacobian), ("the pose", self.rotation)):
            if t is not None and t.device != xyz.device:
                raise ValueError(f"{name}: {what} must live on the device of xyz")
        if xyz.device.type != "cuda":
            raise ValueError(f"{name}: the points must live on the GPU; there is no CPU path")
        posed = torch.empty(m, n, 3, dtype=torch.float32, device=xyz.device)
        if n:
            points = dict(xyz=xyz.contiguous(), labels=labels.contiguous(), count=count,
                          jacobian=None if jacobian is None else jacobian.contiguous(), posed=posed)
            hip.field_pose(self.labels, None, None, None, None, self.commands,
                           dict(rotation=self.rotation, translation=self.translation, status=self.status, depth=self.depth),
                           parts_count=self.count, points=points, phase=hip.FIELD_POSE_POINTS)
        return posed


def _check_points(name: str, xyz, labels, jacobian, a_dim: int) -> int:
    if not torch.is_tensor(xyz) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{name}: xyz must be fp32 [n, 3]")
    n = xyz.shape[0]
    _check_labels(name, labels, n)
    if jacobian is not None and (not torch.is_tensor(jacobian) or jacobian.dtype != torch.float32
                                 or tuple(jacobian.shape) != (n, a_dim, 3)):
        raise ValueError(f"{name}: jacobian must be fp32 [{n}, {a_dim}, 3] or None")
    return n


def _check_twists(name: str, twists):
    """The checks of a FieldTwists that the pose and the inverse kinematics share; ``(K, A)``."""
    if not isinstance(twists, FieldTwists):
        raise ValueError(f"{name}: twists must be a FieldTwists")
    parts = twists.labels
    if not torch.is_tensor(parts) or parts.dtype != torch.int32 or parts.dim() != 1:
        raise ValueError(f"{name}: twists.labels must be int32 [K]")
    k = parts.shape[0]
    if not 1 <= k <= hip.FIELD_TWISTS_MAX_PARTS:
        raise ValueError(f"{name}: the twists must hold 1 to {hip.FIELD_TWISTS_MAX_PARTS} parts (got {k})")
    omega = twists.omega
    if not torch.is_tensor(omega) or omega.dtype != torch.float64 or omega.dim() != 3 or omega.shape[0] != k or omega.shape[2] != 3:
        raise ValueError(f"{name}: twists.omega must be float64 [{k}, A, 3]")
    a_dim = omega.shape[1]
    if not 1 <= a_dim <= hip.MAX_ACTION_DIM:
        raise ValueError(f"{name}: 1 to {hip.MAX_ACTION_DIM} command channels (got {a_dim})")
    for what, t, dtype, shape in (("velocity", twists.velocity, torch.float64, (k, a_dim, 3)),
                                  ("centroid", twists.centroid, torch.float64, (k, 3)), ("status", twists.status, torch.int32, (k,))):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f"{name}: twists.{what} must be {str(dtype).replace('torch.', '')} {list(shape)}")
    return k, a_dim


def _check_links(name: str, twists, joints, tree, k: int, a_dim: int, like: torch.Tensor):
    """The checks of the joints and the tree; ``(parts_count, same, links)``: the twists' count, the (name, tensor) pairs that
    must share a device, and the joints dict of hip.field_pose (None without joints)."""
    if (joints is None) != (tree is None):
        raise ValueError(f"{name}: joints and tree come together or not at all")
    parts_count = _one_int32(name, "twists.count", twists.count, like)
    same = [("twists.labels", twists.labels), ("twists.omega", twists.omega), ("twists.velocity", twists.velocity),
            ("twists.centroid", twists.centroid), ("twists.status", twists.status)]
    links = None
    if joints is not None:
        if not isinstance(joints, FieldJoints):
            raise ValueError(f"{name}: joints must be a FieldJoints")
        if not torch.is_tensor(joints.part_a) or joints.part_a.dtype != torch.int32 or joints.part_a.dim() != 1:
            raise ValueError(f"{name}: joints.part_a must be int32 [J]")
        j = joints.part_a.shape[0]
        if not 1 <= j <= hip.FIELD_JOINTS_MAX:
            raise ValueError(f"{name}: the joints must hold 1 to {hip.FIELD_JOINTS_MAX} rows (got {j})")
        for what, t, dtype, shape in (("part_b", joints.part_b, torch.int32, (j,)), ("anchor", joints.anchor, torch.float64, (j, 3)),
                                      ("omega", joints.omega, torch.float64, (j, a_dim, 3)),
                                      ("velocity", joints.velocity, torch.float64, (j, a_dim, 3))):
            if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape:
                raise ValueError(f"{name}: joints.{what} must be {str(dtype).replace('torch.', '')} {list(shape)}")
        if not isinstance(tree, (tuple, list)) or len(tree) != 2:
            raise ValueError(f"{name}: tree must be (parent, joint_of), as FieldJoints.tree() returns it")
        for what, t in zip(("parent", "joint_of"), tree):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != (k,):
                raise ValueError(f"{name}: tree {what} must be int32 [{k}] (FieldJoints.tree(), not parents())")
        joints_count = _one_int32(name, "joints.count", joints.count, like)
        same += [("joints.part_a", joints.part_a), ("joints.part_b", joints.part_b), ("joints.anchor", joints.anchor),
                 ("joints.omega", joints.omega), ("joints.velocity", joints.velocity), ("tree parent", tree[0]),
                 ("tree joint_of", tree[1])]
        links = dict(part_a=joints.part_a.contiguous(), part_b=joints.part_b.contiguous(), count=joints_count,
                     anchor=joints.anchor.contiguous(), omega=joints.omega.contiguous(), velocity=joints.velocity.contiguous(),
                     parent=tree[0].contiguous(), joint_of=tree[1].contiguous())
    return parts_count, same, links


def _pose(name: str, twists, commands, joints, tree, points=None):
    """The argument checks (under the caller's ``name``) and the launches of part_poses / cloud_pose.  ``points``: None or
    ``(xyz, labels, count, jacobian)``; then the result is ``(FieldPose, posed)``."""
    k, a_dim = _check_twists(name, twists)
    parts, omega = twists.labels, twists.omega
    if not torch.is_tensor(commands) or commands.dtype != torch.float32 or commands.dim() != 2 or commands.shape[1] != a_dim:
        raise ValueError(f"{name}: commands must be fp32 [M, {a_dim}]")
    m = commands.shape[0]
    if not 1 <= m <= hip.FIELD_POSE_MAX_COMMANDS:
        raise ValueError(f"{name}: 1 to {hip.FIELD_POSE_MAX_COMMANDS} commands (got {m})")
    parts_count, same, links = _check_links(name, twists, joints, tree, k, a_dim, commands)
    n = 0
    if points is not None:
        xyz, labels, count, jacobian = points
        n = _check_points(name, xyz, labels, jacobian, a_dim)
        count = _one_int32(name, "count", count, commands)
        same += [("xyz", xyz), ("labels", labels)] + ([] if jacobian is None else [("jacobian", jacobian)])
    for what, t in same:
        if t.device != commands.device:
            raise ValueError(f"{name}: {what} must live on the device of commands")
    if commands.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = commands.device
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    pose = FieldPose(labels=parts, count=twists.count, rotation=torch.empty(m, k, 3, 3, **f64), translation=torch.empty(m, k, 3, **f64),
                     status=torch.empty(k, **i32), depth=torch.empty(k, **i32), commands=commands.contiguous())
    out = dict(rotation=pose.rotation, translation=pose.translation, status=pose.status, depth=pose.depth)
    posed, rows = None, None
    if points is not None:
        posed = torch.empty(m, n, 3, dtype=torch.float32, device=dev)
        if n:
            rows = dict(xyz=xyz.contiguous(), labels=labels.contiguous(), count=count,
                        jacobian=None if jacobian is None else jacobian.contiguous(), posed=posed)
    hip.field_pose(parts.contiguous(), twists.status.contiguous(), twists.centroid.contiguous(), omega.contiguous(),
                   twists.velocity.contiguous(), pose.commands, out, parts_count=parts_count, joints=links, points=rows)
    return pose if points is None else (pose, posed)


def part_poses(twists: FieldTwists, commands: torch.Tensor, *, joints: Optional[FieldJoints] = None, tree=None) -> FieldPose:
    """Where every part goes under each of the M commands ``commands`` ``[M, A]`` (fp32): the rigid motion ``x -> R x + t`` per
    command and part, in double.  With ``joints`` (``cloud_joints``) and ``tree`` (``joints.tree()``:
    parent and joint_of, int32 on the device) a part's motion is the product of the exponentials of the relative twists of
    the joints along its chain, about their anchors, and of the root's own twist about its centroid, the root applied last;
    without them every part moves by the exponential of its own twist about its centroid.  The tree is caller data: a cycle,
    a self-parent, a joint that does not join the two slots or a parent outside the list give the identity and status bit
    2, after a walk of at most K steps.  No atomics, no host read: equal bytes from call to call, capturable."""
    return _pose("part_poses", twists, commands, joints, tree)


def cloud_pose(cloud: FieldPointCloud, labels: torch.Tensor, twists: FieldTwists, commands: torch.Tensor, *,
               joints: Optional[FieldJoints] = None, tree=None, first_order_elsewhere: bool = True):
    """``(FieldPose, posed [M, n, 3] fp32)``: ``part_poses`` and, in the same sequence of launches, the rows of an extracted
    cloud under every command -- ``cloud.xyz``, ``cloud.count`` and ``labels`` ``[n]`` int32, the per-row result of
    ``cloud_components``.  A row of a part of status 0 moves rigidly with it; every other row takes the field's own first-order
    step ``x + sum_a u_a J_a(x)`` from ``cloud.jacobian`` (``first_order_elsewhere=True``) or stays where it is."""
    if not isinstance(cloud, FieldPointCloud):
        raise ValueError("cloud_pose: cloud must be a FieldPointCloud")
    jacobian = cloud.jacobian if first_order_elsewhere else None
    return _pose("cloud_pose", twists, commands, joints, tree, points=(cloud.xyz, labels, cloud.count, jacobian))


# ---- inverse kinematics on the part tree: commands from 3-D point targets ------------------------------------
@dataclass
class FieldCommands:
    """The commands that bring labelled points to 3-D targets (``solve_commands``; include/njf_hip.h: njf_field_commands), one
    per problem: ``commands[m]`` minimises the weighted mean squared distance between the points under the finite pose of
    ``part_poses`` and ``targets[m]``, plus ``(reg / A) |u|^2``, inside the box.  ``commands`` is the iterate itself, on the
    fp32 lattice: ``part_poses(twists, fit.commands, ...)`` reproduces the pose whose ``cost`` is reported.  ``status`` 0 or
    bits: 1 = the problem has no counted row (``commands`` = the clamped init, cost 0), 2 = the starting objective is not
    finite (``commands`` = the clamped init).  ``part_status`` and ``depth`` are those of ``part_poses``; a part whose status is
    not 0 is not in the objective.  ``moments`` are the 23 weighted moments of (point, target) per problem and part about
    the part's centroid: s0, s1 [3], S2 [6], t1 [3], C [9], e -- all the solver reads of the rows."""

    commands: torch.Tensor       # [M, A] fp32
    cost: torch.Tensor           # [M] float64: the mean squared distance at commands
    initial_cost: torch.Tensor   # [M] float64: the mean squared distance at the start
    weight: torch.Tensor         # [M] float64: W_m, the sum of the counted rows' weights
    steps: torch.Tensor          # [M] int32: accepted steps
    gradient: torch.Tensor       # [M, A] float64: the half-gradient with the regulariser at commands
    status: torch.Tensor         # [M] int32
    part_status: torch.Tensor    # [K] int32
    depth: torch.Tensor          # [K] int32
    moments: torch.Tensor        # [M, K, 23] float64

    def rms(self) -> torch.Tensor:
        """``[M]`` float64: the root of the weighted mean squared distance at ``commands``."""
        return self.cost.sqrt()


def _box(name: str, what: str, v, m: int, a_dim: int, like: torch.Tensor, of: str = "targets"):
    """``[M, A]`` fp32 on the device from None, a Python number, or an fp32 tensor ``[A]`` or ``[M, A]``."""
    if v is None:
        return None
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return torch.full((m, a_dim), float(v), dtype=torch.float32, device=like.device)
    if not torch.is_tensor(v) or v.dtype != torch.float32 or tuple(v.shape) not in ((a_dim,), (m, a_dim)):
        raise ValueError(f"{name}: {what} must be fp32 [{a_dim}] or [{m}, {a_dim}]")
    if v.device != like.device:
        raise ValueError(f"{name}: {what} must live on the device of {of}")
    return v.expand(m, a_dim).contiguous()


def _check_solver(name: str, twists, xyz, labels, m: int, n: int, k: int, a_dim: int, like: torch.Tensor, of: str, joints, tree,
                  weights, count, init, lower, upper, reg, iterations, damping):
    """The checks of ``solve_commands`` that follow those of the twists, the points and the targets (``like``, called ``of`` in
    the messages), shared with the registration; ``(parts_count, links, count, lower, upper)``."""
    if weights is not None and (not torch.is_tensor(weights) or weights.dtype != torch.float32
                                or tuple(weights.shape) not in ((n,), (m, n))):
        raise ValueError(f"{name}: weights must be fp32 [{n}] or [{m}, {n}]")
    if init is not None and (not torch.is_tensor(init) or init.dtype != torch.float32 or tuple(init.shape) != (m, a_dim)):
        raise ValueError(f"{name}: init must be fp32 [{m}, {a_dim}]")
    for what, v in (("reg", reg), ("damping", damping)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{name}: {what} must be a number")
    if not reg >= 0.0:
        raise ValueError(f"{name}: reg must be >= 0 (got {reg})")
    if not damping > 0.0:
        raise ValueError(f"{name}: damping must be > 0 (got {damping})")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= hip.FIELD_COMMANDS_MAX_ITERATIONS:
        raise ValueError(f"{name}: iterations must be an integer in [0, {hip.FIELD_COMMANDS_MAX_ITERATIONS}] (got {iterations})")
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)   # noqa: E731
    if number(lower) and number(upper) and lower > upper:
        raise ValueError(f"{name}: lower > upper ({lower} > {upper})")
    lower, upper = _box(name, "lower", lower, m, a_dim, like, of), _box(name, "upper", upper, m, a_dim, like, of)
    parts_count, same, links = _check_links(name, twists, joints, tree, k, a_dim, like)
    count = _one_int32(name, "count", count, like)
    same += [("xyz", xyz), ("labels", labels)] + [(what, t) for what, t in (("weights", weights), ("init", init)) if t is not None]
    for what, t in same:
        if t.device != like.device:
            raise ValueError(f"{name}: {what} must live on the device of {of}")
    return parts_count, links, count, lower, upper


def solve_commands(twists: FieldTwists, xyz: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor, *,
                   joints: Optional[FieldJoints] = None, tree=None, weights: Optional[torch.Tensor] = None,
                   count: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None, lower=None, upper=None,
                   reg: float = 0.0, iterations: int = 20, damping: float = 1e-3) -> FieldCommands:
    """Inverse kinematics on the part tree: for each of the M target sets ``targets`` ``[M, n, 3]`` (fp32)
    of the points ``xyz`` ``[n, 3]`` (fp32) with part labels ``labels`` ``[n]`` (int32), the command whose finite pose --
    ``part_poses`` with the same ``twists``, ``joints`` and ``tree`` -- brings the points to their targets in the weighted
    least-squares sense.  A row counts when it lies below ``count`` (int32 device tensor; None = n), its label is a part of
    pose status 0, its weight (``weights`` fp32 ``[n]`` or ``[M, n]``; None = 1) is finite and positive and its target is finite:
    a NaN target leaves a row unconstrained.  ``init`` ``[M, A]`` (fp32; None = zeros) starts the iteration, ``lower`` and
    ``upper`` (a number, fp32 ``[A]`` or ``[M, A]``) box it, ``reg`` weighs ``|u|^2 / A``.  One pass over the rows forms 23 moments
    per problem and part; the ``iterations`` Levenberg-Marquardt rounds that follow never look at a row again.  In double,
    without atomics or a host read: equal bytes from call to call, capturable."""
    return _solve("solve_commands", twists, xyz, labels, targets, None, False, joints, tree, weights, count, init, lower, upper, reg,
                  iterations, damping)


def _solve(name: str, twists, xyz, labels, targets, information, metric: bool, joints, tree, weights, count, init, lower, upper, reg,
           iterations, damping):
    """``solve_commands`` and, with ``metric``, ``solve_commands_metric``: the checks, the outputs and the launch."""
    k, a_dim = _check_twists(name, twists)
    n = _check_points(name, xyz, labels, None, a_dim)
    if not torch.is_tensor(targets) or targets.dtype != torch.float32 or targets.dim() != 3 or tuple(targets.shape[1:]) != (n, 3):
        raise ValueError(f"{name}: targets must be fp32 [M, {n}, 3]")
    m = targets.shape[0]
    if not 1 <= m <= hip.FIELD_POSE_MAX_COMMANDS:
        raise ValueError(f"{name}: 1 to {hip.FIELD_POSE_MAX_COMMANDS} target sets (got {m})")
    if metric:
        if not torch.is_tensor(information) or information.dtype != torch.float32 \
                or tuple(information.shape) not in ((n, 6), (m, n, 6)):
            raise ValueError(f"{name}: information must be fp32 [{n}, 6] or [{m}, {n}, 6]")
        if information.device != targets.device:
            raise ValueError(f"{name}: information must live on the device of targets")
    parts_count, links, count, lower, upper = _check_solver(name, twists, xyz, labels, m, n, k, a_dim, targets, "targets", joints,
                                                            tree, weights, count, init, lower, upper, reg, iterations, damping)
    if targets.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = targets.device
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    per_part = hip.FIELD_COMMANDS_METRIC_MOMENTS_PER_PART if metric else hip.FIELD_COMMANDS_MOMENTS_PER_PART
    fit = (FieldMetricCommands if metric else FieldCommands)(
        commands=torch.empty(m, a_dim, dtype=torch.float32, device=dev), cost=torch.empty(m, **f64),
        initial_cost=torch.empty(m, **f64), weight=torch.empty(m, **f64), steps=torch.empty(m, **i32),
        gradient=torch.empty(m, a_dim, **f64), status=torch.empty(m, **i32), part_status=torch.empty(k, **i32),
        depth=torch.empty(k, **i32), moments=torch.empty(m, k, per_part, **f64))
    points = dict(xyz=xyz.contiguous(), labels=labels.contiguous(), count=count, targets=targets.contiguous())
    if metric:
        points["information"] = information.contiguous()
    (hip.field_commands_metric if metric else hip.field_commands)(
        twists.labels.contiguous(), twists.status.contiguous(), twists.centroid.contiguous(), twists.omega.contiguous(),
        twists.velocity.contiguous(), points, {f: getattr(fit, f) for f in fit.__dataclass_fields__}, parts_count=parts_count,
        joints=links, weights=None if weights is None else weights.contiguous(), init=None if init is None else init.contiguous(),
        lower=lower, upper=upper, reg=reg, iterations=iterations, damping=damping)
    return fit


def cloud_commands(cloud: FieldPointCloud, labels: torch.Tensor, twists: FieldTwists, targets: torch.Tensor, *,
                   joints: Optional[FieldJoints] = None, tree=None, weights: Optional[torch.Tensor] = None,
                   init: Optional[torch.Tensor] = None, lower=None, upper=None, reg: float = 0.0, iterations: int = 20,
                   damping: float = 1e-3) -> FieldCommands:
    """``solve_commands`` on the rows of an extracted cloud: ``cloud.xyz`` and ``cloud.count`` with ``labels`` ``[n]`` int32, the
    per-row result of ``cloud_components`` -- the inverse of ``cloud_pose``: targets ``[M, n, 3]`` for the cloud's rows in,
    commands out."""
    if not isinstance(cloud, FieldPointCloud):
        raise ValueError("cloud_commands: cloud must be a FieldPointCloud")
    try:
        return solve_commands(twists, cloud.xyz, labels, targets, joints=joints, tree=tree, weights=weights, count=cloud.count,
                              init=init, lower=lower, upper=upper, reg=reg, iterations=iterations, damping=damping)
    except ValueError as err:
        raise ValueError(str(err).replace("solve_commands:", "cloud_commands:", 1)) from None


# ---- registration to an unlabelled cloud: closest points on a cell list ------------------------------------
def cell_grid(lower: Sequence[float], upper: Sequence[float], cell: float) -> FieldGrid:
    """The cell lattice of ``nearest_points`` over the box ``lower`` .. ``upper``: origin = ``lower``, the three steps equal to
    ``cell``, ``dims_c = max(1, ceil((upper_c - lower_c) / cell))`` cells per axis (at most 1,024).  Points outside the box are
    still found: they land in the boundary cells."""
    name = "cell_grid"
    if isinstance(cell, bool) or not isinstance(cell, (int, float)) or not cell > 0.0 or not math.isfinite(cell):
        raise ValueError(f"{name}: cell must be a finite number > 0 (got {cell})")
    try:
        lo, hi = tuple(float(v) for v in lower), tuple(float(v) for v in upper)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: lower and upper have three numbers each") from None
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(v) for v in lo + hi):
        raise ValueError(f"{name}: lower and upper have three finite numbers each")
    if any(u < l for l, u in zip(lo, hi)):
        raise ValueError(f"{name}: lower > upper ({lo} > {hi})")
    dims = tuple(max(1, int(math.ceil((u - l) / cell))) for l, u in zip(lo, hi))
    if max(dims) > hip.FIELD_NEAREST_MAX_DIM:
        raise ValueError(f"{name}: at most {hip.FIELD_NEAREST_MAX_DIM} cells per axis (got {dims}); take a larger cell")
    return FieldGrid(lo, (cell,) * 3, dims)


@dataclass
class FieldNearest:
    """The closest valid observed point of every searched query row (``nearest_points``; include/njf_hip.h: njf_field_nearest),
    per problem: the exact arg-min of ``(dx*dx + dy*dy) + dz*dz`` in fp32, ties to the lowest index, accepted within
    ``max_distance``.  ``matched`` holds the observed point itself or three NaNs -- ``solve_commands``' "this row is free"."""

    index: torch.Tensor       # [M, n] int32: the observed point's row, -1 = none
    distance2: torch.Tensor   # [M, n] fp32: its squared distance, +inf = none
    matched: torch.Tensor     # [M, n, 3] fp32: the point, or NaN
    found: torch.Tensor       # [M] int32: the accepted rows


def _check_cloud_cells(name: str, observed, cells, mq: int = 1, m_other: int = 1, what: str = "observed"):
    """The checks of a cloud and of the lattice it is sorted into, shared by everything that builds the cell list
    (``_check_nearest``, ``voxel_reduce``).  ``(observed [Mo, T, 3], M)``."""
    if not torch.is_tensor(observed) or observed.dtype != torch.float32 or observed.dim() not in (2, 3) or observed.shape[-1] != 3 \
            or observed.shape[-2] < 1:
        raise ValueError(f"{name}: {what} must be fp32 [T, 3] or [Mo, T, 3] with T >= 1")
    observed = observed.reshape(-1, *observed.shape[-2:]) if observed.dim() == 3 else observed[None]
    mo, t = observed.shape[:2]
    m = max(mo, mq, m_other)
    if not 1 <= m <= hip.FIELD_POSE_MAX_COMMANDS or mo < 1 or mq < 1:
        raise ValueError(f"{name}: 1 to {hip.FIELD_POSE_MAX_COMMANDS} problems (got {min(mo, mq, m)} and {m})")
    if mo not in (1, m) or mq not in (1, m):
        raise ValueError(f"{name}: observed and queries hold one set or one per problem (got {mo} and {mq} for {m} problems)")
    if mo * t >= 2 ** 31:
        raise ValueError(f"{name}: Mo * T must stay below 2**31")
    if not isinstance(cells, FieldGrid):
        raise ValueError(f"{name}: cells must be a FieldGrid (cell_grid)")
    cell = cells.step[0]
    if not cell > 0.0 or not math.isfinite(cell) or cells.step[1] != cell or cells.step[2] != cell or not 1.0 / cell < 2.0 ** 127:
        raise ValueError(f"{name}: cells must have three equal steps > 0 (got {cells.step})")
    if max(cells.dims) > hip.FIELD_NEAREST_MAX_DIM:
        raise ValueError(f"{name}: at most {hip.FIELD_NEAREST_MAX_DIM} cells per axis (got {cells.dims})")
    if mo * cells.num_nodes >= 2 ** 31:
        raise ValueError(f"{name}: Mo * the number of cells must stay below 2**31")
    return observed, m


def _check_cloud_count(name: str, what: str, count, mo: int) -> None:
    if count is not None and (not torch.is_tensor(count) or count.dtype != torch.int32 or tuple(count.shape) != (mo,)):
        raise ValueError(f"{name}: {what} must be int32 [{mo}]")


def _check_nearest(name: str, observed, cells, max_distance, observed_count, count, labels, n: int, mq: int, like: torch.Tensor,
                   of: str, m_other: int = 1, reach_name: str = "max_distance"):
    """The checks of the observation, the lattice and the search that ``nearest_points``, ``point_normals`` and the registration
    share; ``like`` (called ``of`` in the messages) rules the device, ``reach_name`` is what the caller calls ``max_distance``.
    ``(observed [Mo, T, 3], M, observed_count, count)``."""
    observed, m = _check_cloud_cells(name, observed, cells, mq, m_other)
    mo, cell = observed.shape[0], cells.step[0]
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float)) or not max_distance > 0.0 \
            or not math.isfinite(max_distance):
        raise ValueError(f"{name}: {reach_name} must be a finite number > 0 (got {max_distance})")
    with np.errstate(over="ignore"):
        reach = float(np.float32(max_distance))          # the kernel's float
    if not reach > 0.0:
        raise ValueError(f"{name}: {reach_name} must be a finite number > 0 (got {max_distance})")
    if not math.isfinite(reach) or not math.isfinite(reach / cell) or math.ceil(reach / cell) + 1 > hip.FIELD_NEAREST_MAX_RINGS:
        raise ValueError(f"{name}: {reach_name} may span at most {hip.FIELD_NEAREST_MAX_RINGS - 1} cells (got {max_distance} for cells "
                         f"of {cell}); take a larger cell")
    _check_cloud_count(name, "observed_count", observed_count, mo)
    count = _one_int32(name, "count", count, like)
    _check_labels(name, labels, n, optional=True)
    for what, v in (("observed", observed), ("observed_count", observed_count), ("labels", labels)):
        if v is not None and v.device != like.device:
            raise ValueError(f"{name}: {what} must live on the device of {of}")
    return observed, m, observed_count, count


def _nearest_outputs(m: int, n: int, dev) -> FieldNearest:
    return FieldNearest(index=torch.empty(m, n, dtype=torch.int32, device=dev), distance2=torch.empty(m, n, dtype=torch.float32, device=dev),
                        matched=torch.empty(m, n, 3, dtype=torch.float32, device=dev), found=torch.empty(m, dtype=torch.int32, device=dev))


def _nearest_launch(observed, queries, cells: FieldGrid, max_distance, m: int, near: Optional[FieldNearest], observed_count, count,
                    labels, phase: int, workspace: torch.Tensor) -> None:
    out = None if near is None else {f: getattr(near, f) for f in near.__dataclass_fields__}
    hip.field_nearest(observed, queries, cells.c_grid(), max_distance, out, m, observed_count=observed_count, count=count,
                      labels=labels, phase=phase, workspace=workspace)


def nearest_points(queries: torch.Tensor, observed: torch.Tensor, cells: FieldGrid, max_distance: float, *,
                   observed_count: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                   labels: Optional[torch.Tensor] = None) -> FieldNearest:
    """For every row of ``queries`` ``[n, 3]`` or ``[Mq, n, 3]`` (fp32) the closest point of the unlabelled cloud ``observed``
    ``[T, 3]`` or ``[Mo, T, 3]`` (fp32) within ``max_distance``: M = max(Mq, Mo) problems, each of Mq and
    Mo 1 or M.  A point is valid below ``observed_count`` (int32 ``[Mo]``; None = T) with finite coordinates; a row is searched
    below ``count`` (one int32 on the device; None = n) with finite coordinates and, with ``labels`` (int32 ``[n]``), a label >=
    0.  The result is the exact arg-min of ``(dx*dx + dy*dy) + dz*dz`` in fp32, ties to the lowest index; ``cells``
    (``cell_grid``) only sets the cost: the points are sorted into its cells and a query walks the rings of cells around its
    own, so it reads the records nearby instead of all T.  Integer atomics only, no host read: equal bytes from call to call,
    capturable."""
    name = "nearest_points"
    if not torch.is_tensor(queries) or queries.dtype != torch.float32 or queries.dim() not in (2, 3) or queries.shape[-1] != 3:
        raise ValueError(f"{name}: queries must be fp32 [n, 3] or [Mq, n, 3]")
    queries = queries if queries.dim() == 3 else queries[None]
    mq, n = queries.shape[:2]
    observed, m, observed_count, count = _check_nearest(name, observed, cells, max_distance, observed_count, count, labels, n, mq,
                                                        queries, "queries")
    if queries.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    near = _nearest_outputs(m, n, queries.device)
    workspace = torch.empty(hip.field_nearest_workspace(observed.shape[0], cells.num_nodes, observed.shape[1]), dtype=torch.int32,
                            device=queries.device)
    _nearest_launch(observed.contiguous(), queries.contiguous(), cells, max_distance, m, near,
                    None if observed_count is None else observed_count.contiguous(), count,
                    None if labels is None else labels.contiguous(), hip.FIELD_NEAREST_ALL, workspace)
    return near


# ---- surface normals of an observed cloud: exact moments on the cell list ---------------------------------
@dataclass
class FieldNormals:
    """The normal, the neighbour count and the surface variation of every searched query row (``point_normals``;
    include/njf_hip.h: njf_field_normals), per problem, from the covariance of the valid observed points within the radius.
    ``moments`` holds the ten integer sums the rest is computed from: ``S0`` (the count), ``S1[3]`` and ``S2[6]`` (``[xx xy xz
    yy yz zz]``) of the offsets quantised to ``radius / 2^18``."""

    normal: torch.Tensor                  # [M, n, 3] fp32: the unit normal, or NaN
    neighbours: torch.Tensor              # [M, n] int32: the points within the radius, 0 for a row that is not searched
    variation: torch.Tensor               # [M, n] fp32: lambda0 / (lambda0 + lambda1 + lambda2) -- 0 on a plane, 1/3 isotropic --, or NaN
    moments: torch.Tensor                 # [M, n, 10] int64
    eigenvalues: Optional[torch.Tensor]   # [M, n, 3] float64, ascending, in the cloud's units (``eigenvalues=True``), or None

    def information(self, max_variation: Optional[float] = None) -> torch.Tensor:
        """``plane_information(normal)`` ``[M, n, 6]`` (fp32, with its floor): what ``register_commands_metric`` takes as
        ``observed_information`` when the rows are the observed points.  A row without a normal gives six NaNs, which
        ``solve_commands_metric`` reads as "this row is free"; so does, with ``max_variation``, a row whose ``variation``
        exceeds it (an edge, a corner, a thin or noisy neighbourhood).  Torch ops on the device, no host read."""
        name = "FieldNormals.information"
        if max_variation is not None and (isinstance(max_variation, bool) or not isinstance(max_variation, (int, float))
                                          or not max_variation >= 0.0):
            raise ValueError(f"{name}: max_variation must be a number >= 0 or None (got {max_variation})")
        info = plane_information(self.normal)
        if max_variation is not None:
            info = torch.where((self.variation <= float(max_variation))[..., None], info, torch.full_like(info, float("nan")))
        return info


def point_normals(queries: Optional[torch.Tensor], observed: torch.Tensor, cells: FieldGrid, radius: float, *,
                  observed_count: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                  viewpoint: Optional[torch.Tensor] = None, min_neighbours: int = 3, eigenvalues: bool = False) -> FieldNormals:
    """For every row of ``queries`` ``[n, 3]`` or ``[Mq, n, 3]`` (fp32; None = the observed points themselves) the surface
    normal of the unlabelled cloud ``observed`` ``[T, 3]`` or ``[Mo, T, 3]`` (fp32) around it: the
    eigenvector of the smallest eigenvalue of the covariance of the valid points within ``radius``, M = max(Mq, Mo, Mv)
    problems, each of Mq, Mo and Mv 1 or M.  A point is valid below ``observed_count`` (int32 ``[Mo]``; None = T) with finite
    coordinates; a row is searched below ``count`` (one int32 on the device; None = n) with finite coordinates; a neighbour
    has ``(ex*ex + ey*ey) + ez*ez <= radius * radius`` in fp32.  A row with fewer than ``min_neighbours`` (>= 3) neighbours, or
    whose neighbours all coincide, has no normal: NaN, which ``information()`` hands on as a free row.  With ``viewpoint``
    (fp32 ``[3]`` or ``[Mv, 3]``) a normal points to the half-space of the viewpoint; without, its largest component is
    positive.  ``cells`` (``cell_grid``) only sets the cost, as for ``nearest_points``, whose cell list this reads: a row visits
    the cells within ``radius`` of its own.  The neighbourhood sums are integers (offsets quantised to ``radius / 2^18``), so
    the order in which the list is read cannot matter: integer atomics only (the build's), no host read, equal bytes from call
    to call, capturable."""
    name = "point_normals"
    if queries is not None and (not torch.is_tensor(queries) or queries.dtype != torch.float32 or queries.dim() not in (2, 3)
                                or queries.shape[-1] != 3):
        raise ValueError(f"{name}: queries must be fp32 [n, 3] or [Mq, n, 3], or None")
    if viewpoint is not None and (not torch.is_tensor(viewpoint) or viewpoint.dtype != torch.float32 or viewpoint.dim() not in (1, 2)
                                  or viewpoint.shape[-1] != 3 or viewpoint.shape[0] < 1):
        raise ValueError(f"{name}: viewpoint must be fp32 [3] or [Mv, 3]")
    viewpoint = viewpoint if viewpoint is None or viewpoint.dim() == 2 else viewpoint[None]
    mv = 1 if viewpoint is None else viewpoint.shape[0]
    if queries is not None:
        queries = queries if queries.dim() == 3 else queries[None]
    like, of = (observed, "observed") if queries is None else (queries, "queries")
    mq, n = (1, 0) if queries is None else queries.shape[:2]
    observed, m, observed_count, count = _check_nearest(name, observed, cells, radius, observed_count, count, None, n, mq, like, of,
                                                        m_other=mv, reach_name="radius")
    if queries is None:
        queries = observed
        mq, n = queries.shape[:2]
    if mv not in (1, m):
        raise ValueError(f"{name}: viewpoint holds one point or one per problem (got {mv} for {m} problems)")
    if observed.shape[1] >= hip.FIELD_NORMALS_MAX_POINTS:
        raise ValueError(f"{name}: T must stay below 2**26")
    if isinstance(min_neighbours, bool) or not isinstance(min_neighbours, int) or not 3 <= min_neighbours < 2 ** 31:
        raise ValueError(f"{name}: min_neighbours must be an integer >= 3 (got {min_neighbours})")
    if not isinstance(eigenvalues, bool):
        raise ValueError(f"{name}: eigenvalues must be True or False (got {eigenvalues})")
    if viewpoint is not None and viewpoint.device != like.device:
        raise ValueError(f"{name}: viewpoint must live on the device of {of}")
    if queries.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = queries.device
    out = FieldNormals(normal=torch.empty(m, n, 3, dtype=torch.float32, device=dev),
                       neighbours=torch.empty(m, n, dtype=torch.int32, device=dev),
                       variation=torch.empty(m, n, dtype=torch.float32, device=dev),
                       moments=torch.empty(m, n, hip.FIELD_NORMALS_MOMENTS_PER_ROW, dtype=torch.int64, device=dev),
                       eigenvalues=torch.empty(m, n, 3, dtype=torch.float64, device=dev) if eigenvalues else None)
    workspace = torch.empty(hip.field_normals_workspace(observed.shape[0], cells.num_nodes, observed.shape[1]), dtype=torch.int32,
                            device=dev)
    hip.field_normals(observed.contiguous(), queries.contiguous(), cells.c_grid(), radius,
                      {f: getattr(out, f) for f in out.__dataclass_fields__}, m,
                      observed_count=None if observed_count is None else observed_count.contiguous(), count=count,
                      viewpoint=None if viewpoint is None else viewpoint.contiguous(), min_neighbours=min_neighbours,
                      phase=hip.FIELD_NORMALS_ALL, workspace=workspace)
    return out


# ---- observed clouds from depth images: back-projection and voxel centroids -------------------------------
@dataclass
class FieldDepthPoints:
    """The world points of depth frames (``depth_points``; include/njf_hip.h: njf_field_depth_points): one row per pixel,
    row-major, the views of a scene one after the other; a pixel that gives no point holds three NaNs, which
    ``nearest_points``, ``point_normals`` and ``voxel_reduce`` skip."""

    points: torch.Tensor      # [B / V, V*H*W, 3] fp32
    kept: torch.Tensor        # [B / V] int32: the pixels that gave a point


def depth_points(depth: torch.Tensor, intrinsics: torch.Tensor, cam2world: torch.Tensor, *, kind: str = "z", near: float = 0.0,
                 far: float = math.inf, max_jump: Optional[float] = None, views_per_scene: int = 1) -> FieldDepthPoints:
    """The back-projection of the depth frames ``depth`` ``[B, H, W]`` (fp32) through the cameras ``intrinsics`` ``[B, 3, 3]``
    (normalised) and ``cam2world`` ``[B, 4, 4]``.  The pixel grid is ``geometry.get_pixel_coordinates``'
    (row-major, pixel centres) and the ray of a pixel ``geometry.full_frame_rays``', bit for bit: origin o, unit direction d,
    camera-space cz.  ``kind="ray"``: the depth is a distance along the unit ray (``Model.forward``'s rendered depth), t =
    depth; ``kind="z"``: it is the camera-space z that depth cameras report, t = depth / cz.  The point is ``o + d * t`` in fp32,
    equal to that torch expression byte for byte.  A pixel is valid when its depth is finite and ``near < depth <= far`` in
    fp32 (``near = 0`` drops a sensor's zeros); with ``max_jump`` (a relative threshold > 0) a valid pixel is dropped as well
    when a 4-neighbour inside the image has a valid depth ``dn`` with ``|depth - dn| > max_jump * min(depth, dn)``: both sides
    of a depth edge go, and with them the "flying" pixels between them.  The ``views_per_scene`` = V consecutive views of a
    scene become one cloud.  Every row is written, NaN where there is no point; no host read, capturable."""
    name = "depth_points"
    if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.dim() != 3 or min(depth.shape) < 1:
        raise ValueError(f"{name}: depth must be fp32 [B, H, W] with B, H, W >= 1")
    b, h, w = depth.shape
    if not torch.is_tensor(intrinsics) or intrinsics.dtype != torch.float32 or tuple(intrinsics.shape) != (b, 3, 3):
        raise ValueError(f"{name}: intrinsics must be fp32 [{b}, 3, 3]")
    if not torch.is_tensor(cam2world) or cam2world.dtype != torch.float32 or tuple(cam2world.shape) != (b, 4, 4):
        raise ValueError(f"{name}: cam2world must be fp32 [{b}, 4, 4]")
    if kind not in hip.FIELD_DEPTH_KINDS:
        raise ValueError(f"{name}: kind must be one of {sorted(hip.FIELD_DEPTH_KINDS)} (got {kind!r})")
    for what, v in (("near", near), ("far", far)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
            raise ValueError(f"{name}: {what} must be a number (got {v})")
    with np.errstate(over="ignore"):
        near32, far32 = float(np.float32(near)), float(np.float32(far))     # the kernel's floats
    if not 0.0 <= near32 < math.inf or not far32 > near32:
        raise ValueError(f"{name}: 0 <= near < far, near finite (got {near} and {far})")
    jump32 = 0.0                                                             # the kernel's "no such test"
    if max_jump is not None:
        if isinstance(max_jump, bool) or not isinstance(max_jump, (int, float)):
            raise ValueError(f"{name}: max_jump must be a finite number > 0 or None (got {max_jump})")
        with np.errstate(over="ignore"):
            jump32 = float(np.float32(max_jump))
        if not 0.0 < jump32 < math.inf:
            raise ValueError(f"{name}: max_jump must be a finite number > 0 or None (got {max_jump})")
    if isinstance(views_per_scene, bool) or not isinstance(views_per_scene, int) or views_per_scene < 1:
        raise ValueError(f"{name}: views_per_scene must be an integer >= 1 (got {views_per_scene})")
    if b % views_per_scene:
        raise ValueError(f"{name}: the batch ({b}) must be a multiple of views_per_scene ({views_per_scene})")
    if b * h * w >= 2 ** 31:
        raise ValueError(f"{name}: B * H * W must stay below 2**31")
    for what, t in (("intrinsics", intrinsics), ("cam2world", cam2world)):
        if t.device != depth.device:
            raise ValueError(f"{name}: {what} must live on the device of depth")
    if depth.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    scenes = b // views_per_scene
    out = FieldDepthPoints(points=torch.empty(scenes, views_per_scene * h * w, 3, dtype=torch.float32, device=depth.device),
                           kept=torch.empty(scenes, dtype=torch.int32, device=depth.device))
    hip.field_depth_points(depth.contiguous(), hip.inverse(intrinsics).contiguous(), cam2world.contiguous(),
                           hip.FIELD_DEPTH_KINDS[kind], near32, far32, jump32, views_per_scene, out.points, out.kept)
    return out


@dataclass
class FieldVoxels:
    """One centroid per kept cell of a lattice (``voxel_reduce``; include/njf_hip.h: njf_field_voxels), per problem, in
    ascending cell index.  ``points`` is a valid ``observed`` with or without ``observed_count=count``: the rows from the count
    on hold NaN (and weight 0, cell -1, sums 0)."""

    points: torch.Tensor      # [M, capacity, 3] fp32: the centroids
    weight: torch.Tensor      # [M, capacity] int32: the points of the cell
    cell: torch.Tensor        # [M, capacity] int32: its index (cx * dims_y + cy) * dims_z + cz
    sums: torch.Tensor        # [M, capacity, 3] int64: the fractional cell coordinates of its points in steps of 2^-20 cells, summed
    count: torch.Tensor       # [M] int32: the TRUE number of kept cells; may exceed the capacity
    outside: torch.Tensor     # [M] int32: the valid points outside the lattice, which are not reduced


def voxel_reduce(points: torch.Tensor, cells: FieldGrid, *, count: Optional[torch.Tensor] = None, min_points: int = 1,
                 capacity: Optional[int] = None) -> FieldVoxels:
    """The cloud ``points`` ``[T, 3]`` or ``[M, T, 3]`` (fp32) thinned to one centroid per occupied cell of ``cells``
    (``cell_grid``), per problem.  A point is valid below ``count`` (int32 ``[M]``; None = T) with finite
    coordinates, and inside when its unclamped cell ``floor((p - origin) / cell)`` lies in the lattice; valid points outside are
    not reduced but counted in ``outside``.  A cell is kept with at least ``min_points`` points (more than 1 removes speckle);
    its centroid is the mean of the points' cell coordinates quantised to 2^-20 cells -- exact integer sums, so the order in
    which the cell list is read cannot matter: equal bytes from call to call, capturable, integer atomics only.  The kept cells
    come in ascending cell index; ``capacity`` (None = min(T, C), which cannot overflow) bounds the rows, ``count`` stays true
    beyond it, and the rows behind the kept ones are NaN: ``points`` goes into ``nearest_points``, ``point_normals`` and the
    registration as it is."""
    name = "voxel_reduce"
    points, m = _check_cloud_cells(name, points, cells, what="points")
    t = points.shape[1]
    _check_cloud_count(name, "count", count, m)
    if isinstance(min_points, bool) or not isinstance(min_points, int) or not 1 <= min_points < 2 ** 31:
        raise ValueError(f"{name}: min_points must be an integer in [1, 2**31) (got {min_points})")
    if capacity is None:
        capacity = min(t, cells.num_nodes)
    elif isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1 or m * capacity >= 2 ** 31:
        raise ValueError(f"{name}: capacity must be an integer >= 1 with M * capacity below 2**31, or None (got {capacity})")
    if count is not None and count.device != points.device:
        raise ValueError(f"{name}: count must live on the device of points")
    if points.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = points.device
    out = FieldVoxels(points=torch.empty(m, capacity, 3, dtype=torch.float32, device=dev),
                      weight=torch.empty(m, capacity, dtype=torch.int32, device=dev),
                      cell=torch.empty(m, capacity, dtype=torch.int32, device=dev),
                      sums=torch.empty(m, capacity, 3, dtype=torch.int64, device=dev),
                      count=torch.empty(m, dtype=torch.int32, device=dev), outside=torch.empty(m, dtype=torch.int32, device=dev))
    hip.field_voxels(points.contiguous(), cells.c_grid(), {f: getattr(out, f) for f in out.__dataclass_fields__},
                     points_count=None if count is None else count.contiguous(), min_points=min_points, phase=hip.FIELD_VOXELS_ALL)
    return out


# ---- which posed rows a depth camera sees: a z-buffer of points -------------------------------------------
@dataclass
class FieldView:
    """The depth cameras that look at a body (``visible_rows``; ``visible_from`` of ``register_commands_visible``): ``intrinsics`` ``[V, 3,
    3]`` (normalised, as ``depth_points`` takes them) and ``cam2world`` ``[V, 4, 4]`` (fp32), images of ``height`` x ``width``.  A
    row is splatted over the ``(2 footprint + 1)^2`` pixels around its own (0 to 4); it is visible when its camera-space z lies
    within ``tolerance * zmin`` of the smallest z in its own pixel and beyond ``near``.  A footprint of 0 lets the far side of a
    body show through the gaps between rows that lie a pixel or more apart."""

    intrinsics: torch.Tensor
    cam2world: torch.Tensor
    height: int
    width: int
    footprint: int = 1
    tolerance: float = 0.01
    near: float = 0.0


@dataclass
class FieldVisibility:
    """What the cameras of a ``FieldView`` see of a point set (``visible_rows``; include/njf_hip.h: njf_field_visible), per
    problem.  ``depth[m]`` ``[V, H, W]`` is the depth image each camera would report and a valid ``depth`` of
    ``depth_points(kind="z")`` with the same cameras: an empty pixel holds 0, which ``near=0`` drops.  ``culled`` is a valid
    ``queries`` of ``nearest_points``: a hidden row holds NaN and is not searched."""

    seen: torch.Tensor        # [M, n] int32: bit v set iff the row is visible in view v
    culled: torch.Tensor      # [M, n, 3] fp32: the point itself where seen != 0, else NaN
    visible: torch.Tensor     # [M] int32: the rows with seen != 0
    depth: torch.Tensor       # [M, V, H, W] fp32: the smallest camera-space z splatted into the pixel, 0 = none
    index: torch.Tensor       # [M, V, H, W] int32: the row that gave it (ties to the lowest), -1 = none
    covered: torch.Tensor     # [M, V] int32: the pixels with a depth
    pixel: torch.Tensor       # [M, V, n] int32: row * W + col of the row's own pixel, -1 = outside the image, behind it, or not read
    z: torch.Tensor           # [M, V, n] fp32: the row's camera-space z, NaN for a row that is not read


def _check_view(name: str, view, like: torch.Tensor, of: str, m: int, n: int, splat: bool = True):
    """The checks of a ``FieldView`` against ``m`` problems of ``n`` rows on the device of ``like`` (called ``of``);
    ``(V, near, tolerance)`` with the two numbers as the kernel's floats.  Without ``splat`` the two fields of the z-buffer,
    ``footprint`` and ``tolerance``, are not read: ``(V, near)``."""
    if not isinstance(view, FieldView):
        raise ValueError(f"{name}: the view must be a FieldView")
    k, c2w = view.intrinsics, view.cam2world
    if not torch.is_tensor(k) or k.dtype != torch.float32 or k.dim() != 3 or tuple(k.shape[1:]) != (3, 3) \
            or not 1 <= k.shape[0] <= hip.FIELD_VISIBLE_MAX_VIEWS:
        raise ValueError(f"{name}: intrinsics must be fp32 [V, 3, 3] with 1 <= V <= {hip.FIELD_VISIBLE_MAX_VIEWS}")
    v = k.shape[0]
    if not torch.is_tensor(c2w) or c2w.dtype != torch.float32 or tuple(c2w.shape) != (v, 4, 4):
        raise ValueError(f"{name}: cam2world must be fp32 [{v}, 4, 4]")
    for what, value in (("height", view.height), ("width", view.width)):
        if isinstance(value, bool) or not isinstance(value, int) or value < 1:
            raise ValueError(f"{name}: {what} must be an integer >= 1 (got {value})")
    f = view.footprint
    if splat and (isinstance(f, bool) or not isinstance(f, int) or not 0 <= f <= hip.FIELD_VISIBLE_MAX_FOOTPRINT):
        raise ValueError(f"{name}: footprint must be an integer in [0, {hip.FIELD_VISIBLE_MAX_FOOTPRINT}] (got {f})")
    floats = []
    for what, value in (("near", view.near), ("tolerance", view.tolerance))[:2 if splat else 1]:
        if isinstance(value, bool) or not isinstance(value, (int, float)) or math.isnan(value):
            raise ValueError(f"{name}: {what} must be a finite number >= 0 (got {value})")
        with np.errstate(over="ignore"):
            value32 = float(np.float32(value))                  # the kernel's float
        if not 0.0 <= value32 < math.inf:
            raise ValueError(f"{name}: {what} must be a finite number >= 0 (got {value})")
        floats.append(value32)
    if m * v * view.height * view.width >= 2 ** 31:
        raise ValueError(f"{name}: M * V * height * width must stay below 2**31")
    if m * v * n >= 2 ** 31:
        raise ValueError(f"{name}: M * V * n must stay below 2**31")
    for what, t in (("intrinsics", k), ("cam2world", c2w)):
        if t.device != like.device:
            raise ValueError(f"{name}: {what} must live on the device of {of}")
    return (v, *floats)


class _Visibility:
    """The launches of ``visible_rows`` for ``m`` problems of ``n`` rows: the world-to-camera matrices (``hip.inverse``) and the
    workspace are made once, ``__call__`` takes the points ``[Mq, n, 3]`` of one round."""

    def __init__(self, view: FieldView, v: int, near: float, tolerance: float, m: int, n: int, dev):
        self.k, self.w2c = view.intrinsics.contiguous(), hip.inverse(view.cam2world).contiguous()
        self.shape, self.m, self.n, self.dev = (v, view.height, view.width), m, n, dev
        self.kw = dict(footprint=view.footprint, near=near, tolerance=tolerance, phase=hip.field_visible_default_phase())
        self.workspace = torch.empty(hip.field_visible_workspace(m, v, view.height, view.width), dtype=torch.int32, device=dev)

    def __call__(self, points: torch.Tensor, count, labels) -> FieldVisibility:
        (v, h, w), m, n = self.shape, self.m, self.n
        i32, f32 = dict(dtype=torch.int32, device=self.dev), dict(dtype=torch.float32, device=self.dev)
        out = FieldVisibility(seen=torch.empty(m, n, **i32), culled=torch.empty(m, n, 3, **f32), visible=torch.empty(m, **i32),
                              depth=torch.empty(m, v, h, w, **f32), index=torch.empty(m, v, h, w, **i32),
                              covered=torch.empty(m, v, **i32), pixel=torch.empty(m, v, n, **i32), z=torch.empty(m, v, n, **f32))
        hip.field_visible(points, self.k, self.w2c, h, w, {f: getattr(out, f) for f in out.__dataclass_fields__}, m, count=count,
                          labels=labels, workspace=self.workspace, **self.kw)
        return out


def visible_rows(points: torch.Tensor, view: FieldView, *, labels: Optional[torch.Tensor] = None,
                 count: Optional[torch.Tensor] = None) -> FieldVisibility:
    """Which rows of ``points`` ``[n, 3]`` or ``[M, n, 3]`` (fp32) the depth cameras of ``view`` see, and
    the depth images they would report.  A row is read below ``count`` (one int32 on the device; None = n) with finite
    coordinates and, with ``labels`` (int32 ``[n]``), a label >= 0 -- ``nearest_points``' searched row.  Every read row in front
    of a camera (z > ``view.near``) is projected by the pinhole model of ``depth_points`` and written over its footprint into a
    z-buffer that keeps the smallest z per pixel, ties to the lowest row; a row is visible in a view when it falls into the
    image and ``z - zmin <= tolerance * zmin`` at its own pixel.  ``FieldVisibility.depth[m]`` is a valid ``depth`` for
    ``depth_points(kind="z")`` with the same cameras; ``culled`` goes into ``nearest_points`` as its queries.  The z-buffer is a
    64-bit integer minimum, so the order of the atomics cannot matter: equal bytes from call to call, no host read, capturable."""
    name = "visible_rows"
    points, (m, n) = _posed_points(name, points, "M")
    if not 1 <= m <= hip.FIELD_POSE_MAX_COMMANDS:
        raise ValueError(f"{name}: 1 to {hip.FIELD_POSE_MAX_COMMANDS} problems (got {m})")
    v, near, tolerance = _check_view(name, view, points, "points", m, n)
    count = _one_int32(name, "count", count, points)
    _check_labels(name, labels, n, optional=True)
    if labels is not None and labels.device != points.device:
        raise ValueError(f"{name}: labels must live on the device of points")
    if points.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    run = _Visibility(view, v, near, tolerance, m, n, points.device)
    return run(points.contiguous(), count, None if labels is None else labels.contiguous())


@dataclass
class FieldRegistration:
    """The commands that bring the parts onto an unlabelled observation (``register_commands``): ``fit`` is the
    ``FieldCommands`` of the last round, ``matches`` the ``FieldNearest`` it solved on; the histories hold every round's
    commands, cost and number of matched rows.  The cost need not fall from round to round: the correspondences change."""

    fit: FieldCommands
    matches: FieldNearest
    commands_history: torch.Tensor   # [R, M, A] fp32: the commands after every round
    cost_history: torch.Tensor       # [R, M] float64
    found_history: torch.Tensor      # [R, M] int32


@dataclass
class FieldVisibleRegistration(FieldRegistration):
    """``FieldRegistration`` of a registration that culls the posed rows by what the cameras see (``register_commands_visible``):
    ``visible_history`` holds the rows seen in every round; ``found_history`` stays the matched rows."""

    visible_history: torch.Tensor    # [R, M] int32


def _registration_outputs(cull, rounds: int, m: int, a_dim: int, dev) -> FieldRegistration:
    histories = dict(fit=None, matches=None, commands_history=torch.empty(rounds, m, a_dim, dtype=torch.float32, device=dev),
                     cost_history=torch.empty(rounds, m, dtype=torch.float64, device=dev),
                     found_history=torch.empty(rounds, m, dtype=torch.int32, device=dev))
    if cull is None:
        return FieldRegistration(**histories)
    return FieldVisibleRegistration(**histories, visible_history=torch.empty(rounds, m, dtype=torch.int32, device=dev))


def register_commands(twists: FieldTwists, xyz: torch.Tensor, labels: torch.Tensor, observed: torch.Tensor, cells: FieldGrid,
                      max_distance: float, *, joints: Optional[FieldJoints] = None, tree=None,
                      observed_count: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                      weights: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None, lower=None, upper=None,
                      reg: float = 0.0, rounds: int = 8, iterations: int = 3, damping: float = 1e-3) -> FieldRegistration:
    """The command that explains an unlabelled observation of the body: closest-point registration of
    the points ``xyz`` ``[n, 3]`` with part labels ``labels`` to the cloud ``observed`` ``[T, 3]`` or ``[Mo, T, 3]``.  The cell list
    of ``observed`` is built once; then, ``rounds`` times from ``u_0 = clamp(init)``: the rows are posed at ``u_r`` (``part_poses``
    and its points launch; rows of no part stay), ``nearest_points`` matches the posed rows of label >= 0 to observed points
    within ``max_distance``, and ``solve_commands(xyz, targets=matched, init=u_r, iterations=iterations)`` gives ``u_{r+1}``.  The
    targets are always targets for the un-posed ``xyz`` and the solver's pose is finite: no pose is ever composed with another.
    M = max(Mo, rows of ``init``) problems; one observation with ``init`` ``[M, A]`` is a multi-start registration, of which the
    caller takes ``fit.cost.argmin()``.  Every other argument is ``solve_commands``'.  No host read: capturable after one
    eager call."""
    return _register("register_commands", None, twists, xyz, labels, observed, cells, max_distance, joints, tree, observed_count, count,
                     weights, init, lower, upper, reg, rounds, iterations, damping)


def _register(name: str, visible_from, twists, xyz, labels, observed, cells, max_distance, joints, tree, observed_count, count, weights,
              init, lower, upper, reg, rounds, iterations, damping):
    """``register_commands`` under the caller's ``name``; with ``visible_from`` (a ``FieldView``) every round culls the posed rows
    before the closest-point query and the result is a ``FieldVisibleRegistration``."""
    k, a_dim = _check_twists(name, twists)
    n = _check_points(name, xyz, labels, None, a_dim)
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= 1000:
        raise ValueError(f"{name}: rounds must be an integer in [1, 1000] (got {rounds})")
    starts = init.shape[0] if torch.is_tensor(init) and init.dim() == 2 else 1
    observed, m, observed_count, count = _check_nearest(name, observed, cells, max_distance, observed_count, count, None, n, 1, xyz,
                                                        "xyz", m_other=max(starts, 1))
    parts_count, links, count, lower_box, upper_box = _check_solver(name, twists, xyz, labels, m, n, k, a_dim, xyz, "xyz", joints, tree,
                                                                    weights, count, init, lower, upper, reg, iterations, damping)
    cull = None if visible_from is None else _check_view(name, visible_from, xyz, "xyz", m, n)
    if xyz.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = xyz.device
    u = torch.zeros(m, a_dim, dtype=torch.float32, device=dev) if init is None else init
    if lower_box is not None:
        u = torch.maximum(u, lower_box)
    if upper_box is not None:
        u = torch.minimum(u, upper_box)
    out = _registration_outputs(cull, rounds, m, a_dim, dev)
    labels_c = labels.contiguous()
    observed_count = None if observed_count is None else observed_count.contiguous()
    if cull is not None:
        cull = _Visibility(visible_from, *cull, m, n, dev)
    workspace = torch.empty(hip.field_nearest_workspace(observed.shape[0], cells.num_nodes, observed.shape[1]), dtype=torch.int32,
                            device=dev)
    _nearest_launch(observed.contiguous(), (1, n), cells, max_distance, m, None, observed_count, None, None, hip.FIELD_NEAREST_BUILD,
                    workspace)
    for r in range(rounds):
        _, posed = _pose(name, twists, u, joints, tree, points=(xyz, labels, count, None))
        if cull is not None:
            seen = cull(posed, count, labels_c)
            out.visible_history[r].copy_(seen.visible)
            posed = seen.culled
        near = _nearest_outputs(m, n, dev)
        _nearest_launch(tuple(observed.shape[:2]), posed, cells, max_distance, m, near, observed_count, count, labels_c,
                        hip.FIELD_NEAREST_QUERY, workspace)
        fit = solve_commands(twists, xyz, labels, near.matched, joints=joints, tree=tree, weights=weights, count=count, init=u,
                             lower=lower, upper=upper, reg=reg, iterations=iterations, damping=damping)
        out.commands_history[r].copy_(fit.commands)
        out.cost_history[r].copy_(fit.cost)
        out.found_history[r].copy_(near.found)
        out.fit, out.matches, u = fit, near, fit.commands
    return out


def cloud_registration(cloud: FieldPointCloud, labels: torch.Tensor, twists: FieldTwists, observed: torch.Tensor,
                       max_distance: float, *, cells: Optional[FieldGrid] = None, joints: Optional[FieldJoints] = None, tree=None,
                       observed_count: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                       init: Optional[torch.Tensor] = None, lower=None, upper=None, reg: float = 0.0, rounds: int = 8,
                       iterations: int = 3, damping: float = 1e-3) -> FieldRegistration:
    """``register_commands`` on the rows of an extracted cloud: ``cloud.xyz`` and ``cloud.count`` with ``labels`` ``[n]`` int32, the
    per-row result of ``cloud_components`` -- the command that explains a second, unlabelled observation of the same body.
    ``cells=None`` takes ``cell_grid`` over the bounds of ``cloud.grid`` with the largest of its steps as the cell."""
    name = "cloud_registration"
    if not isinstance(cloud, FieldPointCloud):
        raise ValueError(f"{name}: cloud must be a FieldPointCloud")
    try:
        if cells is None:
            grid = cloud.grid
            if not isinstance(grid, FieldGrid):
                raise ValueError("register_commands: cloud.grid must be a FieldGrid")
            upper_corner = tuple(o + s * (d - 1) for o, s, d in zip(grid.origin, grid.step, grid.dims))
            cells = cell_grid(tuple(min(o, u) for o, u in zip(grid.origin, upper_corner)),
                              tuple(max(o, u) for o, u in zip(grid.origin, upper_corner)), max(abs(s) for s in grid.step))
        return register_commands(twists, cloud.xyz, labels, observed, cells, max_distance, joints=joints, tree=tree,
                                 observed_count=observed_count, count=cloud.count, weights=weights, init=init, lower=lower,
                                 upper=upper, reg=reg, rounds=rounds, iterations=iterations, damping=damping)
    except ValueError as err:
        raise ValueError(str(err).replace("register_commands:", f"{name}:", 1).replace("cell_grid:", f"{name}:", 1)) from None


# ---- commands from pixel rays and planes: a 3x3 information per target -------------------------------------
@dataclass
class FieldMetricCommands:
    """``FieldCommands`` of the anisotropic objective (``solve_commands_metric``; include/njf_hip.h: njf_field_commands_metric):
    ``cost`` is the weighted mean of ``z^T Q z``, ``z`` the residual of a row and ``Q`` its 3 x 3 information -- a squared
    distance to a ray or a plane when ``Q`` is ``I - d d^T`` or ``n n^T``.  ``moments`` are the 74 weighted moments per problem
    and part about the part's centroid: s0, P [6 x 10], B [3 x 4], e -- all the solver reads of the rows."""

    commands: torch.Tensor       # [M, A] fp32
    cost: torch.Tensor           # [M] float64: the weighted mean of z^T Q z at commands
    initial_cost: torch.Tensor   # [M] float64: the same at the start
    weight: torch.Tensor         # [M] float64: W_m, the sum of the counted rows' weights
    steps: torch.Tensor          # [M] int32: accepted steps
    gradient: torch.Tensor       # [M, A] float64: the half-gradient with the regulariser at commands
    status: torch.Tensor         # [M] int32
    part_status: torch.Tensor    # [K] int32
    depth: torch.Tensor          # [K] int32
    moments: torch.Tensor        # [M, K, 74] float64

    def rms(self) -> torch.Tensor:
        """``[M]`` float64: the root of the weighted mean of ``z^T Q z`` at ``commands``."""
        return self.cost.sqrt()


def solve_commands_metric(twists: FieldTwists, xyz: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor,
                          information: torch.Tensor, *, joints: Optional[FieldJoints] = None, tree=None,
                          weights: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                          init: Optional[torch.Tensor] = None, lower=None, upper=None, reg: float = 0.0, iterations: int = 20,
                          damping: float = 1e-3) -> FieldMetricCommands:
    """``solve_commands`` with an anisotropic error per row: row i of problem m costs ``w z^T Q z``, ``z``
    its residual against ``targets[m, i]`` and ``Q`` the symmetric 3 x 3 ``information`` of the row, fp32 ``[n, 6]`` or ``[M, n,
    6]`` as ``[xx xy xz yy yz zz]``.  ``ray_targets`` gives targets and information for 2-D keypoints in a calibrated camera (a
    pixel holds a point to a ray), ``plane_information`` for point-to-plane matches, ``ray_information`` for a depth camera
    whose noise is larger along the ray; the identity is ``solve_commands``' objective.  ``information`` is not tested for
    definiteness: that is the caller's contract.  A row with a NaN in its information is left out, like one with a NaN
    target; every other argument is ``solve_commands``'.  One pass over the rows forms 74 moments per problem and part; the
    iterations never look at a row again.  In double, without atomics or a host read: equal bytes from call to call,
    capturable."""
    return _solve("solve_commands_metric", twists, xyz, labels, targets, information, True, joints, tree, weights, count, init, lower,
                  upper, reg, iterations, damping)


def cloud_commands_metric(cloud: FieldPointCloud, labels: torch.Tensor, twists: FieldTwists, targets: torch.Tensor,
                          information: torch.Tensor, *, joints: Optional[FieldJoints] = None, tree=None,
                          weights: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None, lower=None, upper=None,
                          reg: float = 0.0, iterations: int = 20, damping: float = 1e-3) -> FieldMetricCommands:
    """``solve_commands_metric`` on the rows of an extracted cloud: ``cloud.xyz`` and ``cloud.count`` with ``labels`` ``[n]`` int32,
    the per-row result of ``cloud_components``."""
    if not isinstance(cloud, FieldPointCloud):
        raise ValueError("cloud_commands_metric: cloud must be a FieldPointCloud")
    try:
        return solve_commands_metric(twists, cloud.xyz, labels, targets, information, joints=joints, tree=tree, weights=weights,
                                     count=cloud.count, init=init, lower=lower, upper=upper, reg=reg, iterations=iterations,
                                     damping=damping)
    except ValueError as err:
        raise ValueError(str(err).replace("solve_commands_metric:", "cloud_commands_metric:", 1)) from None


INFORMATION_FLOOR = 2.0 ** -21   # the least weight in the free directions that keeps the fp32 matrices positive semi-definite


def _outer_plus_identity(name: str, what: str, v, outer: float, identity: float) -> torch.Tensor:
    """``outer u u^T + identity I`` packed ``[..., 6]``, ``u`` the normalised ``v`` ``[..., 3]`` (fp32); arithmetic on the device only."""
    if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() < 1 or v.shape[-1] != 3:
        raise ValueError(f"{name}: {what} must be fp32 [..., 3]")
    x, y, z = (v / torch.linalg.vector_norm(v, dim=-1, keepdim=True)).unbind(-1)
    return torch.stack([outer * (x * x) + identity, outer * (x * y), outer * (x * z), outer * (y * y) + identity, outer * (y * z),
                        outer * (z * z) + identity], dim=-1)


def plane_information(normals: torch.Tensor) -> torch.Tensor:
    """``n n^T`` packed ``[..., 6]`` (``[xx xy xz yy yz zz]``) for ``normals`` ``[..., 3]`` (fp32, normalised here): the information
    of a point-to-plane match -- the residual counts along the normal only and the match may slide in the tangent plane.
    Exactly: ``(1 - f) n n^T + f I`` with ``f = INFORMATION_FLOOR`` = 2^-21, for the reason given at ``ray_information``: the fp32
    ``n n^T`` alone has eigenvalues of either sign near 3e-8 in the plane, where the residual of a slid match is large."""
    return _outer_plus_identity("plane_information", "normals", normals, 1.0 - INFORMATION_FLOOR, INFORMATION_FLOOR)


def ray_information(directions: torch.Tensor, along: float = 0.0) -> torch.Tensor:
    """``I - (1 - along) d d^T`` packed ``[..., 6]`` for ``directions`` ``[..., 3]`` (fp32): weight 1 across the ray and ``along``
    along it.  0 is a pixel ray (the depth is free); a depth camera whose noise along the ray is s times the noise across it
    has ``along = 1 / s^2``; 1 is the identity.  ``along`` below ``INFORMATION_FLOOR`` = 2^-21 counts as that: in fp32 ``|d|^2`` is
    1 only to a few 1e-7, so ``I - d d^T`` itself comes out indefinite along the ray in about every other row, and the residual
    along the ray does not vanish at the solution (``ray_targets``' target is the foot of the UN-posed point).  The cost of a
    good fit then falls below 0, where the solver clamps it and stops telling fits apart (on the planted chain: a command 9e-5
    off).  The floor, with the directions normalised here once more, keeps every matrix positive semi-definite; what it
    adds to the objective is a pull of weight 5e-7 along the ray."""
    name = "ray_information"
    if isinstance(along, bool) or not isinstance(along, (int, float)) or not 0.0 <= along <= 1.0:
        raise ValueError(f"{name}: along must be a number in [0, 1] (got {along})")
    return _outer_plus_identity(name, "directions", directions, -(1.0 - max(float(along), INFORMATION_FLOOR)), 1.0)


def ray_targets(xyz: torch.Tensor, coordinates_xy: torch.Tensor, intrinsics: torch.Tensor, cam2world: torch.Tensor):
    """``(targets [M, n, 3], information [M, n, 6])`` of ``solve_commands_metric`` for 2-D observations of the rows ``xyz`` ``[n,
    3]`` (fp32): ``coordinates_xy`` ``[M, n, 2]`` are the pixels of the rows in the package's normalised convention (x right, y
    down, in [0, 1]; ``geometry.get_pixel_coordinates``), ``intrinsics`` ``[M, 3, 3]`` normalised and ``cam2world`` ``[M, 4, 4]``
    the camera of every problem.  The ray of a pixel is ``geometry.get_world_rays``' (origin o, unit direction d); the
    information is ``ray_information(d)``, ``I - d d^T`` up to its floor, and the target the FOOT of ``xyz[i]`` on its ray, ``o + d (d . (x - o))``.  Any point of the ray
    gives the same objective; the foot keeps the moments at the body's scale however far the camera is.  A row whose
    coordinate is not finite gets a NaN target: it is free.  Several cameras of one problem: concatenate the rows -- ``xyz``
    and ``labels`` repeated once per camera, each copy with its camera's targets and information.  Torch ops on the device
    after the ray launch, no host read."""
    name = "ray_targets"
    if not torch.is_tensor(xyz) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{name}: xyz must be fp32 [n, 3]")
    n = xyz.shape[0]
    if not torch.is_tensor(coordinates_xy) or coordinates_xy.dtype != torch.float32 or coordinates_xy.dim() != 3 \
            or tuple(coordinates_xy.shape[1:]) != (n, 2) or coordinates_xy.shape[0] < 1:
        raise ValueError(f"{name}: coordinates_xy must be fp32 [M, {n}, 2]")
    m = coordinates_xy.shape[0]
    if not torch.is_tensor(intrinsics) or intrinsics.dtype != torch.float32 or tuple(intrinsics.shape) != (m, 3, 3):
        raise ValueError(f"{name}: intrinsics must be fp32 [{m}, 3, 3]")
    if not torch.is_tensor(cam2world) or cam2world.dtype != torch.float32 or tuple(cam2world.shape) != (m, 4, 4):
        raise ValueError(f"{name}: cam2world must be fp32 [{m}, 4, 4]")
    for what, t in (("coordinates_xy", coordinates_xy), ("intrinsics", intrinsics), ("cam2world", cam2world)):
        if t.device != xyz.device:
            raise ValueError(f"{name}: {what} must live on the device of xyz")
    seen = torch.isfinite(coordinates_xy).all(dim=-1, keepdim=True)
    origins, directions = geometry.get_world_rays(torch.where(seen, coordinates_xy, torch.full_like(coordinates_xy, 0.5)), intrinsics,
                                                  cam2world)
    directions = directions / torch.linalg.vector_norm(directions, dim=-1, keepdim=True)
    along = ((xyz[None] - origins) * directions).sum(dim=-1, keepdim=True)
    foot = origins + directions * along
    return torch.where(seen, foot, torch.full_like(foot, float("nan"))), ray_information(directions)


def register_commands_metric(twists: FieldTwists, xyz: torch.Tensor, labels: torch.Tensor, observed: torch.Tensor,
                             observed_information: torch.Tensor, cells: FieldGrid, max_distance: float, *,
                             joints: Optional[FieldJoints] = None, tree=None, observed_count: Optional[torch.Tensor] = None,
                             count: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                             init: Optional[torch.Tensor] = None, lower=None, upper=None, reg: float = 0.0, rounds: int = 8,
                             iterations: int = 3, damping: float = 1e-3) -> FieldRegistration:
    """``register_commands`` with an information per observed point: ``observed_information`` fp32 ``[T,
    6]`` or ``[Mo, T, 6]`` holds the symmetric 3 x 3 of every point of ``observed`` -- ``plane_information`` of the cloud's
    normals makes it point-to-plane registration, in which a match may slide along the surface.  The loop is
    ``register_commands``' with one more step per round: after ``nearest_points``, ``information[m, i] =
    observed_information[mo, max(index[m, i], 0)]`` (a torch gather; a row without a match is free through its NaN target), and
    ``solve_commands_metric`` takes the place of ``solve_commands``.  The correspondences stay the Euclidean arg-min.  Returns a
    ``FieldRegistration`` whose ``fit`` is a ``FieldMetricCommands``.  No host read: capturable after one eager call."""
    return _register_metric("register_commands_metric", None, twists, xyz, labels, observed, observed_information, cells, max_distance,
                            joints, tree, observed_count, count, weights, init, lower, upper, reg, rounds, iterations, damping)


def _register_metric(name: str, visible_from, twists, xyz, labels, observed, observed_information, cells, max_distance, joints, tree,
                     observed_count, count, weights, init, lower, upper, reg, rounds, iterations, damping):
    """``register_commands_metric`` under the caller's ``name``, with ``_register``'s ``visible_from``."""
    k, a_dim = _check_twists(name, twists)
    n = _check_points(name, xyz, labels, None, a_dim)
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= 1000:
        raise ValueError(f"{name}: rounds must be an integer in [1, 1000] (got {rounds})")
    starts = init.shape[0] if torch.is_tensor(init) and init.dim() == 2 else 1
    observed, m, observed_count, count = _check_nearest(name, observed, cells, max_distance, observed_count, count, None, n, 1, xyz,
                                                        "xyz", m_other=max(starts, 1))
    mo, t = observed.shape[:2]
    if not torch.is_tensor(observed_information) or observed_information.dtype != torch.float32 \
            or tuple(observed_information.shape) not in ((t, 6), (mo, t, 6)):
        raise ValueError(f"{name}: observed_information must be fp32 [{t}, 6] or [{mo}, {t}, 6]")
    if observed_information.device != xyz.device:
        raise ValueError(f"{name}: observed_information must live on the device of xyz")
    parts_count, links, count, lower_box, upper_box = _check_solver(name, twists, xyz, labels, m, n, k, a_dim, xyz, "xyz", joints, tree,
                                                                    weights, count, init, lower, upper, reg, iterations, damping)
    cull = None if visible_from is None else _check_view(name, visible_from, xyz, "xyz", m, n)
    if xyz.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = xyz.device
    u = torch.zeros(m, a_dim, dtype=torch.float32, device=dev) if init is None else init
    if lower_box is not None:
        u = torch.maximum(u, lower_box)
    if upper_box is not None:
        u = torch.minimum(u, upper_box)
    out = _registration_outputs(cull, rounds, m, a_dim, dev)
    labels_c = labels.contiguous()
    observed_count = None if observed_count is None else observed_count.contiguous()
    if cull is not None:
        cull = _Visibility(visible_from, *cull, m, n, dev)
    source = observed_information.reshape(-1, t, 6).expand(m, t, 6)          # [T, 6] or Mo = 1: one table for every problem
    workspace = torch.empty(hip.field_nearest_workspace(mo, cells.num_nodes, t), dtype=torch.int32, device=dev)
    _nearest_launch(observed.contiguous(), (1, n), cells, max_distance, m, None, observed_count, None, None, hip.FIELD_NEAREST_BUILD,
                    workspace)
    for r in range(rounds):
        _, posed = _pose(name, twists, u, joints, tree, points=(xyz, labels, count, None))
        if cull is not None:
            seen = cull(posed, count, labels_c)
            out.visible_history[r].copy_(seen.visible)
            posed = seen.culled
        near = _nearest_outputs(m, n, dev)
        _nearest_launch((mo, t), posed, cells, max_distance, m, near, observed_count, count, labels_c, hip.FIELD_NEAREST_QUERY,
                        workspace)
        information = torch.gather(source, 1, near.index.clamp_min(0).long()[:, :, None].expand(m, n, 6))
        fit = solve_commands_metric(twists, xyz, labels, near.matched, information, joints=joints, tree=tree, weights=weights,
                                    count=count, init=u, lower=lower, upper=upper, reg=reg, iterations=iterations, damping=damping)
        out.commands_history[r].copy_(fit.commands)
        out.cost_history[r].copy_(fit.cost)
        out.found_history[r].copy_(near.found)
        out.fit, out.matches, u = fit, near, fit.commands
    return out


def cloud_registration_metric(cloud: FieldPointCloud, labels: torch.Tensor, twists: FieldTwists, observed: torch.Tensor,
                              observed_information: torch.Tensor, max_distance: float, *, cells: Optional[FieldGrid] = None,
                              joints: Optional[FieldJoints] = None, tree=None, observed_count: Optional[torch.Tensor] = None,
                              weights: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None, lower=None, upper=None,
                              reg: float = 0.0, rounds: int = 8, iterations: int = 3, damping: float = 1e-3) -> FieldRegistration:
    """``register_commands_metric`` on the rows of an extracted cloud, as ``cloud_registration`` is ``register_commands`` on
    them; ``cells=None`` takes ``cell_grid`` over the bounds of ``cloud.grid`` with the largest of its steps as the cell."""
    name = "cloud_registration_metric"
    if not isinstance(cloud, FieldPointCloud):
        raise ValueError(f"{name}: cloud must be a FieldPointCloud")
    try:
        if cells is None:
            cells = _cloud_cells(cloud, "register_commands_metric")
        return register_commands_metric(twists, cloud.xyz, labels, observed, observed_information, cells, max_distance,
                                        joints=joints, tree=tree, observed_count=observed_count, count=cloud.count, weights=weights,
                                        init=init, lower=lower, upper=upper, reg=reg, rounds=rounds, iterations=iterations,
                                        damping=damping)
    except ValueError as err:
        raise ValueError(str(err).replace("register_commands_metric:", f"{name}:", 1).replace("cell_grid:", f"{name}:", 1)) from None


def register_commands_visible(twists: FieldTwists, xyz: torch.Tensor, labels: torch.Tensor, observed: torch.Tensor, cells: FieldGrid,
                              max_distance: float, visible_from: FieldView, *, observed_information: Optional[torch.Tensor] = None,
                              joints: Optional[FieldJoints] = None, tree=None, observed_count: Optional[torch.Tensor] = None,
                              count: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                              init: Optional[torch.Tensor] = None, lower=None, upper=None, reg: float = 0.0, rounds: int = 8,
                              iterations: int = 3, damping: float = 1e-3) -> FieldVisibleRegistration:
    """``register_commands`` to an observation that depth cameras made: ``visible_from`` is the ``FieldView``
    of those cameras, and every round goes pose, ``visible_rows`` of the posed rows (with the query's labels and count),
    ``nearest_points`` on its ``culled`` rows instead of the posed rows, solve -- a row the cameras do not see at ``u_r`` is free
    in that round, so the WHOLE body can be registered to a depth image, which shows one side of it.  With
    ``observed_information`` (``register_commands_metric``'s, fp32 ``[T, 6]`` or ``[Mo, T, 6]``) the loop is
    ``register_commands_metric``'s.  Every other argument is ``register_commands``'; the result adds ``visible_history``, the rows
    seen in every round.  The workspace of the z-buffer is allocated once; no host read: capturable after one eager call."""
    name = "register_commands_visible"
    if not isinstance(visible_from, FieldView):
        raise ValueError(f"{name}: the view must be a FieldView")
    if observed_information is None:
        return _register(name, visible_from, twists, xyz, labels, observed, cells, max_distance, joints, tree, observed_count, count,
                         weights, init, lower, upper, reg, rounds, iterations, damping)
    return _register_metric(name, visible_from, twists, xyz, labels, observed, observed_information, cells, max_distance, joints, tree,
                            observed_count, count, weights, init, lower, upper, reg, rounds, iterations, damping)


def cloud_registration_visible(cloud: FieldPointCloud, labels: torch.Tensor, twists: FieldTwists, observed: torch.Tensor,
                               max_distance: float, visible_from: FieldView, *, observed_information: Optional[torch.Tensor] = None,
                               cells: Optional[FieldGrid] = None, joints: Optional[FieldJoints] = None, tree=None,
                               observed_count: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                               init: Optional[torch.Tensor] = None, lower=None, upper=None, reg: float = 0.0, rounds: int = 8,
                               iterations: int = 3, damping: float = 1e-3) -> FieldVisibleRegistration:
    """``register_commands_visible`` on the rows of an extracted cloud, as ``cloud_registration`` is ``register_commands`` on them;
    ``cells=None`` takes ``cell_grid`` over the bounds of ``cloud.grid`` with the largest of its steps as the cell."""
    name = "cloud_registration_visible"
    if not isinstance(cloud, FieldPointCloud):
        raise ValueError(f"{name}: cloud must be a FieldPointCloud")
    try:
        if cells is None:
            cells = _cloud_cells(cloud, "register_commands_visible")
        return register_commands_visible(twists, cloud.xyz, labels, observed, cells, max_distance, visible_from,
                                         observed_information=observed_information, joints=joints, tree=tree,
                                         observed_count=observed_count, count=cloud.count, weights=weights, init=init, lower=lower,
                                         upper=upper, reg=reg, rounds=rounds, iterations=iterations, damping=damping)
    except ValueError as err:
        raise ValueError(str(err).replace("register_commands_visible:", f"{name}:", 1).replace("cell_grid:", f"{name}:", 1)) from None


def _cloud_cells(cloud: FieldPointCloud, name: str) -> FieldGrid:
    """``cell_grid`` over the bounds of ``cloud.grid`` with the largest of its steps as the cell."""
    grid = cloud.grid
    if not isinstance(grid, FieldGrid):
        raise ValueError(f"{name}: cloud.grid must be a FieldGrid")
    upper_corner = tuple(o + s * (d - 1) for o, s, d in zip(grid.origin, grid.step, grid.dims))
    return cell_grid(tuple(min(o, u) for o, u in zip(grid.origin, upper_corner)),
                     tuple(max(o, u) for o, u in zip(grid.origin, upper_corner)), max(abs(s) for s in grid.step))


# ---- posed rows against a depth frame by projection: occlusion, free space, window match --------------------
@dataclass
class FieldFrameMatches(FieldNearest):
    """``FieldNearest`` of a match by projection into an organised depth frame (``frame_matches``; include/njf_hip.h:
    njf_field_frame): ``index`` is a row ``v * H * W + row * W + col`` of the frame.  ``state[m, v, i]`` says how row i agrees with
    the frame at its own pixel in view v -- 0 outside the image (or not read), 1 no return there, 2 in front of what the camera
    saw (free space), 3 on it, 4 behind it (hidden by the scene) --, ``states[m, c]`` counts the (v, i) pairs of code c."""

    state: torch.Tensor       # [M, V, n] int32: hip.FIELD_FRAME_OUTSIDE .. FIELD_FRAME_BEHIND
    states: torch.Tensor      # [M, 5] int32: the (v, i) pairs per code
    pixel: torch.Tensor       # [M, V, n] int32: FieldVisibility.pixel
    z: torch.Tensor           # [M, V, n] fp32: FieldVisibility.z

    def explained(self) -> torch.Tensor:
        """``[M]`` float64: ON / (ON + IN_FRONT + NO_RETURN) of ``states`` -- the share of the rows the cameras should see that
        sit where they saw a surface; NaN when no row is in an image and not hidden."""
        s = self.states.to(torch.float64)
        on = s[:, hip.FIELD_FRAME_ON]
        return on / (on + s[:, hip.FIELD_FRAME_IN_FRONT] + s[:, hip.FIELD_FRAME_NO_RETURN])


@dataclass
class FieldFrameRegistration(FieldVisibleRegistration):
    """``FieldVisibleRegistration`` of a registration to an organised depth frame (``register_commands_frame``): ``matches`` is a
    ``FieldFrameMatches``, ``states_history`` holds its ``states`` of every round."""

    states_history: torch.Tensor     # [R, M, 5] int32


def _check_frame(name: str, frame, view, max_distance, reach, tolerance, keep_hidden, count, labels, n: int, mq: int, like: torch.Tensor,
                 of: str, m_other: int = 1):
    """The checks of the frame, the cameras and the window search that ``frame_matches`` and the registrations to a frame share;
    ``like`` (called ``of``) rules the device.  ``(frame [Mo, V H W, 3], M, V, near, tolerance, count)``, the numbers as the
    kernel's floats."""
    if not torch.is_tensor(frame) or frame.dtype != torch.float32 or frame.dim() not in (2, 3) or frame.shape[-1] != 3 \
            or frame.shape[-2] < 1:
        raise ValueError(f"{name}: frame must be fp32 [T, 3] or [Mo, T, 3] with T >= 1")
    frame = frame if frame.dim() == 3 else frame[None]
    mo, t = frame.shape[:2]
    m = max(mo, mq, m_other)
    if not 1 <= m <= hip.FIELD_POSE_MAX_COMMANDS or mo < 1 or mq < 1:
        raise ValueError(f"{name}: 1 to {hip.FIELD_POSE_MAX_COMMANDS} problems (got {min(mo, mq, m)} and {m})")
    if mo not in (1, m) or mq not in (1, m):
        raise ValueError(f"{name}: frame and points hold one set or one per problem (got {mo} and {mq} for {m} problems)")
    v, near = _check_view(name, view, like, of, m, n, splat=False)
    if v * view.height * view.width != t:
        raise ValueError(f"{name}: frame must hold V * height * width = {v * view.height * view.width} rows (got {t})")
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float)) or math.isnan(max_distance):
        raise ValueError(f"{name}: max_distance must be a finite number >= 0 (got {max_distance})")
    with np.errstate(over="ignore"):
        if not 0.0 <= float(np.float32(max_distance)) < math.inf:              # the kernel's float
            raise ValueError(f"{name}: max_distance must be a finite number >= 0 (got {max_distance})")
    if isinstance(reach, bool) or not isinstance(reach, int) or not 0 <= reach <= hip.FIELD_FRAME_MAX_REACH:
        raise ValueError(f"{name}: reach must be an integer in [0, {hip.FIELD_FRAME_MAX_REACH}] (got {reach})")
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or math.isnan(tolerance):
        raise ValueError(f"{name}: tolerance must be a finite number >= 0 (got {tolerance})")
    with np.errstate(over="ignore"):
        tolerance32 = float(np.float32(tolerance))
    if not 0.0 <= tolerance32 < math.inf:
        raise ValueError(f"{name}: tolerance must be a finite number >= 0 (got {tolerance})")
    if not isinstance(keep_hidden, bool):
        raise ValueError(f"{name}: keep_hidden must be a bool (got {keep_hidden})")
    count = _one_int32(name, "count", count, like)
    _check_labels(name, labels, n, optional=True)
    for what, value in (("frame", frame), ("labels", labels)):
        if value is not None and value.device != like.device:
            raise ValueError(f"{name}: {what} must live on the device of {of}")
    return frame, m, v, near, tolerance32, count


class _FrameMatch:
    """The launch of ``frame_matches`` for ``m`` problems of ``n`` rows: the world-to-camera matrices (``hip.inverse``) are made
    once, ``__call__`` takes the points ``[Mq, n, 3]`` of one round."""

    def __init__(self, frame: torch.Tensor, view: FieldView, v: int, near: float, tolerance: float, max_distance: float, reach: int,
                 keep_hidden: bool, m: int, n: int, dev):
        self.frame, self.k, self.w2c = frame.contiguous(), view.intrinsics.contiguous(), hip.inverse(view.cam2world).contiguous()
        self.shape, self.m, self.n, self.dev = (v, view.height, view.width), m, n, dev
        self.kw = dict(reach=reach, near=near, tolerance=tolerance,
                       phase=hip.FIELD_FRAME_MATCH | (hip.FIELD_FRAME_KEEP_HIDDEN if keep_hidden else 0))
        self.max_distance = max_distance

    def __call__(self, points: torch.Tensor, count, labels) -> FieldFrameMatches:
        (v, h, w), m, n = self.shape, self.m, self.n
        i32, f32 = dict(dtype=torch.int32, device=self.dev), dict(dtype=torch.float32, device=self.dev)
        out = FieldFrameMatches(index=torch.empty(m, n, **i32), distance2=torch.empty(m, n, **f32), matched=torch.empty(m, n, 3, **f32),
                                found=torch.empty(m, **i32), state=torch.empty(m, v, n, **i32),
                                states=torch.empty(m, hip.FIELD_FRAME_STATES, **i32), pixel=torch.empty(m, v, n, **i32),
                                z=torch.empty(m, v, n, **f32))
        hip.field_frame(points, self.frame, self.k, self.w2c, h, w, self.max_distance, {f: getattr(out, f) for f in out.__dataclass_fields__},
                        m, count=count, labels=labels, **self.kw)
        return out


def frame_matches(points: torch.Tensor, frame: torch.Tensor, view: FieldView, max_distance: float, *, reach: int = 4,
                  tolerance: float = 0.02, keep_hidden: bool = False, labels: Optional[torch.Tensor] = None,
                  count: Optional[torch.Tensor] = None) -> FieldFrameMatches:
    """The rows of ``points`` ``[n, 3]`` or ``[Mq, n, 3]`` (fp32) against the depth frame the cameras of ``view`` made (DESIGN.md
    section 26): ``frame`` ``[V H W, 3]`` or ``[Mo, V H W, 3]`` (fp32) is the ORGANISED cloud of ``depth_points`` for the V views of
    a scene -- row ``v H W + row W + col`` is the point of that pixel, NaN where it gave none.  M = max(Mq, Mo) problems, each of
    Mq and Mo 1 or M.  A row (read as ``visible_rows`` reads it, and projected by the same code: ``pixel`` and ``z`` are its bits)
    is classified in every view against the frame's point at its own pixel, whose camera-space z is ``zo``: no return there, in
    front of it (``zo - z > tolerance * zo``: the row floats where the camera saw through), behind it (``z - zo > tolerance *
    zo``: the scene hides it) or on it.  A row is then matched to the closest frame point -- ``nearest_points``' distance and tie
    rule -- among the pixels within ``reach`` (0 to 8) of its own, over all views in which it is inside the image and, unless
    ``keep_hidden``, not behind the frame; accepted within ``max_distance``.  The window must cover the displacement between the
    posed row and its counterpart, in pixels: a row that moved further finds a worse point or none.  ``view.footprint`` and
    ``view.tolerance`` are not read.  No cell list, no workspace, integer atomics only, no host read: equal bytes from call to
    call, capturable."""
    name = "frame_matches"
    points, (mq, n) = _posed_points(name, points, "Mq")
    frame, m, v, near, tolerance, count = _check_frame(name, frame, view, max_distance, reach, tolerance, keep_hidden, count, labels, n,
                                                       mq, points, "points")
    if points.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    run = _FrameMatch(frame, view, v, near, tolerance, max_distance, reach, keep_hidden, m, n, points.device)
    return run(points.contiguous(), count, None if labels is None else labels.contiguous())


def register_commands_frame(twists: FieldTwists, xyz: torch.Tensor, labels: torch.Tensor, frame: torch.Tensor, max_distance: float,
                            view: FieldView, *, observed_information: Optional[torch.Tensor] = None, reach: int = 4,
                            tolerance: float = 0.02, keep_hidden: bool = False, joints: Optional[FieldJoints] = None, tree=None,
                            count: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                            init: Optional[torch.Tensor] = None, lower=None, upper=None, reg: float = 0.0, rounds: int = 8,
                            iterations: int = 3, damping: float = 1e-3) -> FieldFrameRegistration:
    """``register_commands_visible`` to the depth frame itself instead of to its points as an unordered set (DESIGN.md section
    26): ``frame`` is ``frame_matches``' organised cloud of the cameras of ``view``.  Every round goes pose, ``visible_rows`` of the
    posed rows (what the BODY hides; ``view.footprint`` and ``view.tolerance``), ``frame_matches`` on its ``culled`` rows (what the
    SCENE hides, with ``reach``, ``tolerance`` and ``keep_hidden``) instead of the cell-list query, solve.  A row behind a foreign
    object is free instead of being pulled onto that object.  With ``observed_information`` (fp32 ``[V H W, 6]`` or ``[Mo, V H W,
    6]``, indexed by frame row) the loop is ``register_commands_metric``'s.  There is no lattice, no build and no workspace
    beyond the z-buffer's.  The result adds ``states_history``; ``matches.explained()`` of the last round says how much of what
    the cameras should see of the fit they did see.  No host read: capturable after one eager call."""
    name = "register_commands_frame"
    k, a_dim = _check_twists(name, twists)
    n = _check_points(name, xyz, labels, None, a_dim)
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= 1000:
        raise ValueError(f"{name}: rounds must be an integer in [1, 1000] (got {rounds})")
    starts = init.shape[0] if torch.is_tensor(init) and init.dim() == 2 else 1
    frame, m, v, near, tolerance32, count = _check_frame(name, frame, view, max_distance, reach, tolerance, keep_hidden, count, None, n, 1,
                                                         xyz, "xyz", m_other=max(starts, 1))
    cull = _check_view(name, view, xyz, "xyz", m, n)
    mo, t = frame.shape[:2]
    metric = observed_information is not None
    if metric:
        if not torch.is_tensor(observed_information) or observed_information.dtype != torch.float32 \
                or tuple(observed_information.shape) not in ((t, 6), (mo, t, 6)):
            raise ValueError(f"{name}: observed_information must be fp32 [{t}, 6] or [{mo}, {t}, 6]")
        if observed_information.device != xyz.device:
            raise ValueError(f"{name}: observed_information must live on the device of xyz")
    parts_count, links, count, lower_box, upper_box = _check_solver(name, twists, xyz, labels, m, n, k, a_dim, xyz, "xyz", joints, tree,
                                                                    weights, count, init, lower, upper, reg, iterations, damping)
    if xyz.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = xyz.device
    u = torch.zeros(m, a_dim, dtype=torch.float32, device=dev) if init is None else init
    if lower_box is not None:
        u = torch.maximum(u, lower_box)
    if upper_box is not None:
        u = torch.minimum(u, upper_box)
    base = _registration_outputs(cull, rounds, m, a_dim, dev)
    out = FieldFrameRegistration(**{f: getattr(base, f) for f in base.__dataclass_fields__},
                                 states_history=torch.empty(rounds, m, hip.FIELD_FRAME_STATES, dtype=torch.int32, device=dev))
    labels_c = labels.contiguous()
    cull = _Visibility(view, *cull, m, n, dev)
    match = _FrameMatch(frame, view, v, near, tolerance32, max_distance, reach, keep_hidden, m, n, dev)
    source = observed_information.reshape(-1, t, 6).expand(m, t, 6) if metric else None
    solver = dict(joints=joints, tree=tree, weights=weights, count=count, lower=lower, upper=upper, reg=reg, iterations=iterations,
                  damping=damping)
    for r in range(rounds):
        _, posed = _pose(name, twists, u, joints, tree, points=(xyz, labels, count, None))
        seen = cull(posed, count, labels_c)
        near_r = match(seen.culled, count, labels_c)
        if metric:
            information = torch.gather(source, 1, near_r.index.clamp_min(0).long()[:, :, None].expand(m, n, 6))
            fit = solve_commands_metric(twists, xyz, labels, near_r.matched, information, init=u, **solver)
        else:
            fit = solve_commands(twists, xyz, labels, near_r.matched, init=u, **solver)
        out.commands_history[r].copy_(fit.commands)
        out.cost_history[r].copy_(fit.cost)
        out.found_history[r].copy_(near_r.found)
        out.visible_history[r].copy_(seen.visible)
        out.states_history[r].copy_(near_r.states)
        out.fit, out.matches, u = fit, near_r, fit.commands
    return out


def cloud_registration_frame(cloud: FieldPointCloud, labels: torch.Tensor, twists: FieldTwists, frame: torch.Tensor, max_distance: float,
                             view: FieldView, *, observed_information: Optional[torch.Tensor] = None, reach: int = 4,
                             tolerance: float = 0.02, keep_hidden: bool = False, joints: Optional[FieldJoints] = None, tree=None,
                             weights: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None, lower=None, upper=None,
                             reg: float = 0.0, rounds: int = 8, iterations: int = 3, damping: float = 1e-3) -> FieldFrameRegistration:
    """``register_commands_frame`` on the rows of an extracted cloud, as ``cloud_registration`` is ``register_commands`` on them:
    ``cloud.xyz`` and ``cloud.count`` with ``labels`` ``[n]`` int32, the per-row result of ``cloud_components``."""
    name = "cloud_registration_frame"
    if not isinstance(cloud, FieldPointCloud):
        raise ValueError(f"{name}: cloud must be a FieldPointCloud")
    try:
        return register_commands_frame(twists, cloud.xyz, labels, frame, max_distance, view, observed_information=observed_information,
                                       reach=reach, tolerance=tolerance, keep_hidden=keep_hidden, joints=joints, tree=tree,
                                       count=cloud.count, weights=weights, init=init, lower=lower, upper=upper, reg=reg, rounds=rounds,
                                       iterations=iterations, damping=damping)
    except ValueError as err:
        raise ValueError(str(err).replace("register_commands_frame:", f"{name}:", 1)) from None


# ---- depth frames fused into a truncated signed distance -----------------------------------------------------
@dataclass
class FieldDistance:
    """A truncated signed distance on the nodes of ``grid``, fused from depth frames (``fuse_depth``; include/njf_hip.h:
    njf_field_tsdf), per problem: ``values`` is positive in the free space the cameras saw through, negative behind the surface,
    clipped to ``truncation`` in front of it and not observed further than ``truncation`` behind it; ``weight`` is the number of
    views that contributed to the node (at most ``max_weight``), 0 where none did -- ``values`` is NaN there."""

    grid: FieldGrid
    truncation: float         # the kernel's float
    values: torch.Tensor      # [M, N] fp32
    weight: torch.Tensor      # [M, N] fp32
    known: torch.Tensor       # [M] int32: the nodes with weight > 0

    def mesh(self, **capacities) -> "FieldMesh":
        """The fused surface: ``mesh_from_values`` of ``-values`` at 0 over the nodes with a weight (inside = behind the surface);
        ``max_vertices`` and ``max_triangles`` as there."""
        return mesh_from_values(self.grid, -self.values, 0.0, valid=self.weight > 0, **capacities)


@dataclass
class FieldClearance:
    """A ``FieldDistance`` at the rows of a point set (``sample_distance``; include/njf_hip.h: njf_field_tsdf_sample): ``state[m, i]``
    is 0 for a row outside the grid (or not read), 1 where a corner of its cell was never observed, 2 where ``distance`` and
    ``gradient`` -- the trilinear interpolant and its exact derivative -- are known; they are NaN otherwise."""

    state: torch.Tensor       # [M, n] int32: hip.FIELD_TSDF_OUTSIDE, _UNKNOWN, _KNOWN
    distance: torch.Tensor    # [M, n] fp32
    gradient: torch.Tensor    # [M, n, 3] fp32
    states: torch.Tensor      # [M, 3] int32: the rows per code

    def cost(self) -> torch.Tensor:
        """``[M]`` float64: the mean of ``|distance|`` over the KNOWN rows -- how far the rows lie from the fused surface, rows in
        observed free space included; NaN with no KNOWN row."""
        known = self.state == hip.FIELD_TSDF_KNOWN
        total = torch.where(known, self.distance.to(torch.float64).abs(), 0.0).sum(dim=1)
        return total / known.sum(dim=1).to(torch.float64)

    def surface_targets(self, points: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(targets [M, n, 3], information [M, n, 6])`` for ``solve_commands_metric``: the foot of every KNOWN row of ``points``
        (``[n, 3]`` or ``[Mq, n, 3]``, the sampled points) on the surface along the gradient, ``x - distance g / (g . g)``, and
        ``plane_information(g / |g|)``; NaN -- the solver's "row left out" -- for rows that are not KNOWN or have ``g . g == 0``."""
        name = "FieldClearance.surface_targets"
        m, n = self.state.shape
        if not torch.is_tensor(points) or points.dtype != torch.float32 or points.dim() not in (2, 3) or points.shape[-1] != 3 \
                or points.shape[-2] != n or (points.dim() == 3 and points.shape[0] not in (1, m)):
            raise ValueError(f"{name}: points must be fp32 [{n}, 3] or [Mq, {n}, 3] with Mq 1 or {m}")
        if points.device != self.state.device:
            raise ValueError(f"{name}: points must live on the device of the sample")
        g = self.gradient
        gg = (g * g).sum(dim=-1, keepdim=True)
        ok = (self.state == hip.FIELD_TSDF_KNOWN)[..., None] & (gg > 0)
        nan = torch.full((), math.nan, dtype=torch.float32, device=g.device)
        targets = torch.where(ok, points - self.distance[..., None] * g / gg, nan)
        return targets, torch.where(ok, plane_information(torch.where(ok, g, nan)), nan)


def _check_positive(name: str, what: str, value, finite: bool) -> float:
    """``value`` as the kernel's float: a number > 0, finite when ``finite``."""
    rule = f"{name}: {what} must be a {'finite ' if finite else ''}number > 0"
    if isinstance(value, bool) or not isinstance(value, (int, float)) or math.isnan(value):
        raise ValueError(f"{rule} (got {value})")
    with np.errstate(over="ignore"):
        value32 = float(np.float32(value))
    if not value32 > 0.0 or (finite and value32 == math.inf):
        raise ValueError(f"{rule} (got {value})")
    return value32


def fuse_depth(grid: FieldGrid, depth: torch.Tensor, view: FieldView, truncation: float, *, far: float = math.inf,
               max_weight: float = math.inf, into: Optional[FieldDistance] = None) -> FieldDistance:
    """The depth images ``depth`` ``[V, H, W]`` or ``[M, V, H, W]`` (fp32, camera-space z: ``depth_points``' ``kind="z"``,
    ``FieldVisibility.depth``) of the cameras of ``view`` fused into a truncated signed distance on ``grid``.
    Every node is projected into every view by the code ``visible_rows`` projects rows with; where it falls on a pixel with
    ``view.near < d <= far`` it sees ``s = d - z``: free space in front of the surface when positive, and nothing when it lies
    further than ``truncation`` behind it.  The views that see it add ``min(s, truncation)`` to a running mean whose weight is the
    number of views, held at ``max_weight`` so that an old frame fades.  ``into`` -- an earlier result on the same grid, with the
    same truncation and M -- is updated in place and returned; a node no view sees keeps its state, NaN with weight 0 at first.
    ``view.footprint`` and ``view.tolerance`` are not read.  One launch, one integer atomic per workgroup, no host read: equal bytes
    from call to call, capturable."""
    name = "fuse_depth"
    if not isinstance(grid, FieldGrid):
        raise ValueError(f"{name}: grid must be a FieldGrid")
    if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.dim() not in (3, 4):
        raise ValueError(f"{name}: depth must be fp32 [V, H, W] or [M, V, H, W]")
    depth = depth if depth.dim() == 4 else depth[None]
    m = depth.shape[0]
    if not 1 <= m <= hip.FIELD_POSE_MAX_COMMANDS:
        raise ValueError(f"{name}: 1 to {hip.FIELD_POSE_MAX_COMMANDS} problems (got {m})")
    v, near = _check_view(name, view, depth, "depth", m, 0, splat=False)
    if tuple(depth.shape[1:]) != (v, view.height, view.width):
        raise ValueError(f"{name}: depth must hold [{v}, {view.height}, {view.width}] images (got {tuple(depth.shape[1:])})")
    truncation = _check_positive(name, "truncation", truncation, True)
    max_weight = _check_positive(name, "max_weight", max_weight, False)
    if isinstance(far, bool) or not isinstance(far, (int, float)) or math.isnan(far):
        raise ValueError(f"{name}: far must be a number > near (got {far})")
    with np.errstate(over="ignore"):
        far = float(np.float32(far))
    if not far > near:
        raise ValueError(f"{name}: far must be a number > near (got {far} and {near})")
    nodes = grid.num_nodes
    if m * nodes >= 2 ** 31:
        raise ValueError(f"{name}: M * nodes must stay below 2**31")
    if into is not None:
        if not isinstance(into, FieldDistance):
            raise ValueError(f"{name}: into must be a FieldDistance")
        if into.grid != grid or into.truncation != truncation:
            raise ValueError(f"{name}: into must be of the same grid and truncation")
        for what, t, shape in (("values", into.values, (m, nodes)), ("weight", into.weight, (m, nodes)), ("known", into.known, (m,))):
            if not torch.is_tensor(t) or t.dtype != (torch.int32 if what == "known" else torch.float32) or tuple(t.shape) != shape \
                    or not t.is_contiguous():
                raise ValueError(f"{name}: into.{what} must be a contiguous {'int32' if what == 'known' else 'fp32'} {list(shape)}")
            if t.device != depth.device:
                raise ValueError(f"{name}: into.{what} must live on the device of depth")
    if depth.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = depth.device
    out = into if into is not None else FieldDistance(
        grid=grid, truncation=truncation, values=torch.empty(m, nodes, dtype=torch.float32, device=dev),
        weight=torch.empty(m, nodes, dtype=torch.float32, device=dev), known=torch.empty(m, dtype=torch.int32, device=dev))
    hip.field_tsdf(grid.c_grid(), depth.contiguous(), view.intrinsics.contiguous(), hip.inverse(view.cam2world).contiguous(), truncation,
                   dict(values=out.values, weight=out.weight, known=out.known), near=near, far=far, max_weight=max_weight,
                   values_in=None if into is None else into.values, weight_in=None if into is None else into.weight)
    return out


def sample_distance(points: torch.Tensor, field: FieldDistance, *, labels: Optional[torch.Tensor] = None,
                    count: Optional[torch.Tensor] = None) -> FieldClearance:
    """The fused distance ``field`` (``fuse_depth``) and its gradient at the rows of ``points`` ``[n, 3]`` or ``[Mq, n, 3]`` (fp32):
    M = max(Mq, Mf) problems, Mq and the field's Mf each 1 or M.  A row is read as ``visible_rows`` reads it (below ``count``, finite,
    of a label >= 0); a read row inside the grid's box lies in one cell, and where all eight corners of that cell have a weight the
    trilinear interpolant of their values is its ``distance`` and the exact derivative of that interpolant its ``gradient`` --
    which points away from the surface, into free space.  ``FieldClearance.cost()`` ranks poses: a row in observed free space pays
    its distance to the surface.  One launch, integer atomics only, no host read: equal bytes from call to call, capturable."""
    name = "sample_distance"
    points, (mq, n) = _posed_points(name, points, "Mq")
    if not isinstance(field, FieldDistance) or not isinstance(field.grid, FieldGrid):
        raise ValueError(f"{name}: field must be a FieldDistance")
    grid = field.grid
    if any(d < 2 for d in grid.dims) or not all(0.0 < s < math.inf for s in grid.step):
        raise ValueError(f"{name}: the field's grid needs two nodes or more and a finite step > 0 on every axis "
                         f"(got dims {grid.dims}, step {grid.step})")
    for what, t in (("values", field.values), ("weight", field.weight)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != grid.num_nodes:
            raise ValueError(f"{name}: field.{what} must be fp32 [Mf, {grid.num_nodes}]")
    mf = field.values.shape[0]
    if field.weight.shape[0] != mf:
        raise ValueError(f"{name}: field.values and field.weight must hold the same problems")
    m = max(mq, mf)
    if not 1 <= m <= hip.FIELD_POSE_MAX_COMMANDS or mq < 1 or mf < 1:
        raise ValueError(f"{name}: 1 to {hip.FIELD_POSE_MAX_COMMANDS} problems (got {min(mq, mf, m)} and {m})")
    if mq not in (1, m) or mf not in (1, m):
        raise ValueError(f"{name}: field and points hold one set or one per problem (got {mf} and {mq} for {m} problems)")
    if m * n >= 2 ** 31:
        raise ValueError(f"{name}: M * n must stay below 2**31")
    count = _one_int32(name, "count", count, points)
    _check_labels(name, labels, n, optional=True)
    for what, t in (("field.values", field.values), ("field.weight", field.weight), ("labels", labels)):
        if t is not None and t.device != points.device:
            raise ValueError(f"{name}: {what} must live on the device of points")
    if points.device.type != "cuda":
        raise ValueError(f"{name}: the tensors must live on the GPU; there is no CPU path")
    dev = points.device
    out = FieldClearance(state=torch.empty(m, n, dtype=torch.int32, device=dev), distance=torch.empty(m, n, dtype=torch.float32, device=dev),
                         gradient=torch.empty(m, n, 3, dtype=torch.float32, device=dev),
                         states=torch.empty(m, hip.FIELD_TSDF_STATES, dtype=torch.int32, device=dev))
    hip.field_tsdf_sample(points.contiguous(), grid.c_grid(), field.values.contiguous(), field.weight.contiguous(),
                          {f: getattr(out, f) for f in out.__dataclass_fields__}, m, count=count,
                          labels=None if labels is None else labels.contiguous())
    return out


# ---- coarse-to-fine band ----------------------------------------------------------------------------------
@dataclass
class FieldBand:
    """The nodes of a fine grid near anything a coarse look at the field found occupied (``band_from_values``; the ``coarse``
    keyword of extract_field / extract_mesh): ``block_active[b, j]`` says that block j (k^3 cells) of element b lies within
    ``dilate`` coarse nodes of a hit, ``band[b, n]`` that node n lies in (or on the faces of) an active block; ``index`` holds
    the ascending global indices of the band nodes -- exactly sized from an eager call, padded to the capacity otherwise --
    and ``count`` their TRUE number."""

    coarse_grid: FieldGrid
    block_active: torch.Tensor   # [B, Nb] uint8
    band: torch.Tensor           # [B, N] uint8
    index: torch.Tensor          # [n] int32 global index b*N + n
    count: torch.Tensor          # [1] int32


def coarse_grid(grid: FieldGrid, coarse: int) -> FieldGrid:
    """The grid of every ``coarse``-th node of ``grid`` per axis (``coarse`` in 2, 4, 8, 16; every axis of ``grid`` needs
    ``(n - 1) % coarse == 0`` and ``n >= coarse + 1``): same origin, step ``coarse * step`` -- exact, a power of two -- so
    coarse node j has the very coordinates of fine node ``coarse * j``."""
    m = hip.field_band_blocks(grid.dims, coarse)
    step = tuple(coarse * s for s in grid.step)
    if any(float(np.float32(s)) != s for s in step):
        raise ValueError(f"coarse_grid: {coarse} * step is not an fp32 (step {grid.step})")
    return FieldGrid(grid.origin, step, tuple(mc + 1 for mc in m))


def _check_band_arguments(name: str, grid: FieldGrid, coarse, coarse_threshold, dilate, default_threshold=None):
    """The coarse threshold as a float (None without ``coarse``); ValueError on a bad factor, grid, dilation or threshold."""
    if coarse is None:
        if coarse_threshold is not None:
            raise ValueError(f"{name}: coarse_threshold has no meaning without coarse")
        return None
    hip.field_band_blocks(grid.dims, coarse)
    if isinstance(dilate, bool) or not isinstance(dilate, int) or not 0 <= dilate <= hip.FIELD_BAND_MAX_DILATE:
        raise ValueError(f"{name}: coarse_dilate must be 0, 1 or 2 (got {dilate!r})")
    threshold = default_threshold if coarse_threshold is None else coarse_threshold
    if threshold is None or not math.isfinite(float(threshold)):
        raise ValueError(f"{name}: coarse_threshold must be finite")
    return float(threshold)


def _band(grid: FieldGrid, coarse: int, values: torch.Tensor, threshold: float, valid, dilate: int, capacity: Optional[int]):
    """The four band launches on coarse ``values`` [B, M].  ``capacity`` None: one host read (the count), ``index`` exactly
    sized; else no host read and ``index`` padded (or cut) to the capacity."""
    cgrid = coarse_grid(grid, coarse)
    b, dev = values.shape[0], values.device
    m = hip.field_band_blocks(grid.dims, coarse)
    u8 = dict(dtype=torch.uint8, device=dev)
    band = FieldBand(coarse_grid=cgrid, block_active=torch.empty(b, m[0] * m[1] * m[2], **u8),
                     band=torch.empty(b, grid.num_nodes, **u8),
                     index=torch.empty(b * grid.num_nodes if capacity is None else capacity, dtype=torch.int32, device=dev),
                     count=torch.empty(1, dtype=torch.int32, device=dev))
    hip.field_band(grid.c_grid(), coarse, dilate, b, values.reshape(-1), threshold, band.block_active, band.band, band.index,
                   band.count, coarse_valid=valid)
    if capacity is None:
        band.index = band.index[:int(band.count.item())]
    return band


def band_from_values(grid: FieldGrid, coarse: int, coarse_values: torch.Tensor, coarse_threshold: float, *,
                     coarse_valid: Optional[torch.Tensor] = None, dilate: int = 1, max_nodes: Optional[int] = None) -> FieldBand:
    """The band of any scalar on the coarse grid, without the networks: ``coarse_values`` ``[B, M]`` fp32
    on the GPU, M the node count of ``coarse_grid(grid, coarse)``.  A coarse node is a HIT iff it is valid (``coarse_valid``
    ``[B, M]`` bool / uint8) and ``coarse_values >= coarse_threshold`` (NaN is none); a block of ``coarse``^3 cells is active iff
    a hit lies among its corners or within ``dilate`` (0, 1, 2) coarse nodes of them; the band is every fine node in or on an
    active block.  ``max_nodes=None``: one host read, ``index`` exactly sized.  ``max_nodes=M``: no host synchronisation,
    ``index`` holds the first M band nodes and ``count`` their true number."""
    hip.field_band_blocks(grid.dims, coarse)
    threshold = _check_band_arguments("band_from_values", grid, coarse, coarse_threshold, dilate)
    cgrid = coarse_grid(grid, coarse)
    if (not torch.is_tensor(coarse_values) or coarse_values.dim() != 2 or coarse_values.dtype != torch.float32
            or coarse_values.shape[1] != cgrid.num_nodes):
        raise ValueError(f"band_from_values: coarse_values must be fp32 [B, {cgrid.num_nodes}]")
    if coarse_values.shape[0] < 1 or coarse_values.shape[0] * grid.num_nodes >= 2 ** 31:
        raise ValueError("band_from_values: batch * nx*ny*nz must stay below 2**31")
    if max_nodes is not None and (isinstance(max_nodes, bool) or not isinstance(max_nodes, int) or max_nodes < 1):
        raise ValueError(f"band_from_values: max_nodes must be an integer >= 1 (got {max_nodes!r})")
    if coarse_valid is not None:
        if (not torch.is_tensor(coarse_valid) or coarse_valid.dtype not in (torch.bool, torch.uint8)
                or coarse_valid.shape != coarse_values.shape):
            raise ValueError(f"band_from_values: coarse_valid must be bool or uint8 {tuple(coarse_values.shape)}")
        if coarse_valid.device != coarse_values.device:
            raise ValueError("band_from_values: coarse_valid and coarse_values must live on the same device")
        coarse_valid = coarse_valid.contiguous()
    if coarse_values.device.type != "cuda":
        raise ValueError("band_from_values: coarse_values must live on the GPU; there is no CPU path")
    return _band(grid, coarse, coarse_values.contiguous(), threshold, coarse_valid, dilate, max_nodes)


def band_leaks(grid: FieldGrid, band: torch.Tensor, index: torch.Tensor, count: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[1]`` int32 on the device: how many of the inside nodes ``index`` (ascending int32 global indices; the first ``count``
    of them with a device count, all without) have a neighbour along one of the seven edge directions of the Kuhn tetrahedra,
    in either sign, inside the grid and the same batch element, that is not in ``band`` (``[B, N]`` bool / uint8).  0 proves
    that every connected component the band touches lies wholly in it, with all of its surface edges; the reverse does not
    hold.  No host read."""
    if not torch.is_tensor(band) or band.dim() != 2 or band.dtype not in (torch.bool, torch.uint8) or band.shape[1] != grid.num_nodes:
        raise ValueError(f"band_leaks: band must be bool or uint8 [B, {grid.num_nodes}]")
    if band.shape[0] < 1 or band.shape[0] * grid.num_nodes >= 2 ** 31:
        raise ValueError("band_leaks: batch * nx*ny*nz must stay below 2**31")
    if not torch.is_tensor(index) or index.dim() != 1 or index.dtype != torch.int32:
        raise ValueError("band_leaks: index must be int32 [n]")
    if count is not None and (not torch.is_tensor(count) or count.dtype != torch.int32 or count.numel() != 1):
        raise ValueError("band_leaks: count must be one int32")
    if band.device.type != "cuda" or index.device != band.device:
        raise ValueError("band_leaks: band and index must live on one GPU; there is no CPU path")
    return _leaks(grid, band.contiguous(), index.contiguous(), count, index.shape[0])


def _leaks(grid: FieldGrid, band: torch.Tensor, index: torch.Tensor, count, extent: int) -> torch.Tensor:
    leaks = torch.empty(1, dtype=torch.int32, device=band.device)
    hip.field_band_leaks(grid.c_grid(), band.shape[0], band, index, count, extent, leaks)
    return leaks


def _extraction_band(model, enc, grid: FieldGrid, cams, coarse: int, threshold: float, dilate: int, eager: bool, views: int = 1,
                     mode: str = "mean", min_views: int = 1, in_frustum: bool = True) -> FieldBand:
    """The band of an extraction: the dense density-only pass on the coarse grid (a coarse node's density is the value the
    dense fine pass gives at that node), for scenes of several views their fusion on the coarse grid, the band launches.  The
    capacity forms keep the list at B*N entries (4 bytes per node) and read nothing on the host."""
    dec = model.decoder
    cgrid = coarse_grid(grid, coarse)
    b = enc.extrinsics.shape[0]
    fmap, goffs, w, bd, _, _ = _decoder_arguments(model, enc.features)
    values = torch.empty(b, cgrid.num_nodes, dtype=torch.float32, device=enc.features.device)
    hip.field_forward(cgrid.c_grid(), None, None, b * cgrid.num_nodes, cams, fmap, mode=1, w_all=w, b_density=bd,
                      density=values.reshape(-1), precision=dec.precision, **goffs)
    valid = None
    if views > 1:
        values, _, valid = _fuse(cgrid, values, cams if in_frustum else None, views, mode, min_views)
    return _band(grid, coarse, values, threshold, valid, dilate, None if eager else (b // views) * grid.num_nodes)


def _banded_values(model, enc, grid: FieldGrid, cams, band: FieldBand, in_frustum: bool, eager: bool, views: int = 1):
    """What replaces the dense density pass: the per-view density [B, N] with the decoder's value at the band nodes (with
    ``in_frustum``: at those the view sees) and 0 elsewhere -- nodes the band makes invalid downstream -- and the list the
    values were computed on, as (index, device count, extent, compact values)."""
    dec = model.decoder
    dev = enc.features.device
    b, nodes = enc.extrinsics.shape[0], grid.num_nodes
    cg = grid.c_grid()
    index, count, extent = band.index, None if eager else band.count, band.index.shape[0]
    if views > 1:
        index, count = _per_view(index, count, nodes, views)
        extent *= views
    values = torch.zeros(b, nodes, dtype=torch.float32, device=dev)
    compact = torch.empty(extent, dtype=torch.float32, device=dev)
    if extent > 0:
        if in_frustum:
            # the ordered frustum selection on the list: its count stays on the device, the launches keep the list's extent
            seen, seen_count = torch.empty(extent, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
            hip.field_select(cg, b, extent, seen, seen_count, cams=cams, indices=index.contiguous(), count=count)
            index, count = seen, seen_count
        fmap, goffs, w, bd, _, _ = _decoder_arguments(model, enc.features)
        index = index.contiguous()
        hip.field_forward(cg, index, count, extent, cams, fmap, mode=1, w_all=w, b_density=bd, density=compact,
                          precision=dec.precision, **goffs)
        hip.field_scatter(compact, index, count, extent, values)
    return values, (index, count, extent, compact)


def _inside_leaks(grid: FieldGrid, batch: int, band: FieldBand, values: torch.Tensor, threshold: float, index=None, count=None,
                  extent: Optional[int] = None) -> torch.Tensor:
    """band_leaks of the nodes with ``values >= threshold``: ``values`` compact on the list (index, count, extent), or dense
    [batch, N] (then with -inf at every node that is invalid or outside the band) without one."""
    dev = values.device
    total = batch * grid.num_nodes
    extent = total if index is None else extent
    if extent == 0:
        return torch.zeros(1, dtype=torch.int32, device=dev)
    inside, inside_count = torch.empty(extent, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    hip.field_select(grid.c_grid(), batch, extent, inside, inside_count, values=values.reshape(-1), threshold=threshold,
                     indices=index, count=count)
    return _leaks(grid, band.band, inside, inside_count, extent)


def _rows(index: torch.Tensor, rows: int) -> torch.Tensor:
    """The first ``rows`` entries of a list, padded with zeros where it is shorter (rows past a device count are unspecified)."""
    if index.shape[0] >= rows:
        return index[:rows]
    return torch.cat([index, index.new_zeros(rows - index.shape[0])])


class _Stage:
    """The running list of the pipeline: (indices, device count, launch extent).  Eager extraction reads the count after each
    selection to size the next launch exactly; a capture-safe one keeps every intermediate list at B*N entries (4 bytes per
    node) and lets the kernels read the count on the device."""

    def __init__(self, total: int):
        self.indices: Optional[torch.Tensor] = None
        self.count: Optional[torch.Tensor] = None
        self.extent = total


@torch.no_grad()
def extract_field(model, pixel_encoding: PixelEncoding, grid: FieldGrid, density_threshold: float, *,
                  cull: Optional[float] = None, proposal_level: int = -1, in_frustum: bool = True,
                  view_direction: Optional[Sequence[float]] = None, want_color: bool = True, want_jacobian: bool = True,
                  max_points: Optional[int] = None, views_per_scene: int = 1, fuse: str = "mean",
                  min_views: int = 1, min_component_nodes: Optional[int] = None, largest_only: bool = False,
                  connectivity: int = 6, coarse: Optional[int] = None, coarse_threshold: Optional[float] = None,
                  coarse_dilate: int = 1) -> FieldPointCloud:
    """Every node of ``grid`` -- per context image of ``pixel_encoding`` -- that

    1. (``in_frustum``) projects inside the context image with positive camera depth,
    2. (``cull`` is not None) has ``proposal_density >= cull`` for ``model.proposal_networks[proposal_level]``,
    3. has ``decoder_density >= density_threshold`` (the density ``Model.compute_density`` returns),

    with its density, colour (view direction (0, 0, 1) as ``compute_density`` uses, or ``view_direction``) and Jacobian
    ``[A, 3]``, in ascending global index.  ``max_points=None``: exactly sized tensors, one host read of a device count per
    selection stage.  ``max_points=M``: no host synchronisation (safe inside ``torch.cuda.graph``), tensors padded to M rows
    and ``count`` = the true number of survivors (the rows stored are the first M of them).

    ``views_per_scene=V > 1``: the context images are B / V scenes of V consecutive calibrated views in one world frame, and
    ONE cloud per scene comes back (``_extract_field_fused``): ``index`` is the fused global index
    ``g*N + n``, ``density`` the ``fuse`` ("mean", "min", "max") of the views that see the node, colour and Jacobian the
    density-weighted mean over those views, ``views`` their bitmask.  A node needs ``min_views`` views that see it.

    ``min_component_nodes=K`` and / or ``largest_only``: the survivors of the density selection are
    labelled into connected components (``connectivity`` 6 or 14, among the survivors of one batch element / scene) on the
    device, and only the rows of the components of at least K nodes -- ``largest_only``: of the largest of them, ties to the
    smallest label -- are kept, by the same ordered selection; the coordinate pass and the full decoder pass run on the kept
    rows only, ``stage_counts`` / ``stage_names`` get a ``"components"`` entry, and the capacity form leaves the status word of
    the labelling in the attribute ``components_status`` of the result.  With both off nothing changes.

    ``coarse=k`` (2, 4, 8, 16): the density network first runs on every k-th node per axis (every axis of
    ``grid`` needs ``(n - 1) % k == 0``), and the fine pipeline only on the BAND: the nodes in or on a block of k^3 cells that
    has a coarse node with ``density >= coarse_threshold`` (default: ``density_threshold``; lower it for parts thinner than k
    nodes) among its corners or within ``coarse_dilate`` (0, 1, 2) coarse nodes of them.  The result is that of the same call
    without ``coarse`` in which the nodes outside the band are additionally invalid; ``stage_counts`` / ``stage_names`` get a
    leading ``"band"`` entry, and the result carries the attributes ``band_count`` (int32 ``[1]``, the true number of band
    nodes) and ``band_leaks`` (int32 ``[1]``: the survivors of the density selection with a neighbour outside the band -- 0
    proves that every body the band touches lies wholly in it; a body that no coarse node hits within ``(coarse_dilate + 1) *
    k`` nodes is missed silently).  ``coarse=None`` changes nothing."""
    dec = model.decoder
    if not isinstance(dec, ActionDecoderJacobian):
        raise TypeError("extract_field needs one of the fused action decoders")
    _check_fusion_arguments("extract_field", pixel_encoding.extrinsics.shape[0], views_per_scene, fuse, min_views)
    _check_component_arguments("extract_field", connectivity, min_component_nodes)
    coarse_threshold = _check_band_arguments("extract_field", grid, coarse, coarse_threshold, coarse_dilate, density_threshold)
    filtering = min_component_nodes is not None or bool(largest_only)
    if views_per_scene > 1 and cull is not None:
        raise ValueError("extract_field: cull with views_per_scene > 1 has no single meaning (a proposal cull is per view)")
    is_flow = isinstance(dec, ActionDecoderFlowMlp)
    if want_jacobian and is_flow:
        raise NotImplementedError("flow_mlp predicts the scene flow directly; it has no Jacobian")
    if not math.isfinite(float(density_threshold)) or (cull is not None and not math.isfinite(float(cull))):
        raise ValueError("extract_field: thresholds must be finite")
    if max_points is not None and max_points < 1:
        raise ValueError("extract_field: max_points must be >= 1")
    if view_direction is not None and len(view_direction) != 3:
        raise ValueError("extract_field: view_direction has three components")
    feats = pixel_encoding.features
    dev = feats.device
    b = pixel_encoding.extrinsics.shape[0]
    total = b * grid.num_nodes
    if total >= 2 ** 31:
        raise ValueError("extract_field: batch * nx*ny*nz must stay below 2**31")
    cg = grid.c_grid()
    eager = max_points is None
    if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        # the hoisted maps are cached per feature tensor: a capture must CONTAIN the projection, or a replay on refilled
        # features would read the map of the image that was there when it was recorded
        model.reset_image_cache()
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    cams = _cameras(pixel_encoding, False, action_dim=dec.kernel_action_dim if want_jacobian else None)
    if views_per_scene > 1:
        return _extract_field_fused(model, pixel_encoding, grid, float(density_threshold), cams, in_frustum, view_direction,
                                    want_color, want_jacobian, max_points, views_per_scene, fuse, min_views,
                                    (connectivity, min_component_nodes, bool(largest_only)) if filtering else None,
                                    None if coarse is None else (coarse, coarse_threshold, coarse_dilate))
    stage = _Stage(total)
    counts, names = [], []
    band, leaks = None, None
    if coarse is not None:
        # the pipeline starts from the band list instead of the identity
        band = _extraction_band(model, pixel_encoding, grid, cams, coarse, coarse_threshold, coarse_dilate, eager)
        counts.append(band.count)
        names.append("band")
        stage.indices, stage.extent = band.index, band.index.shape[0]
        stage.count = None if eager else band.count
        leaks = torch.zeros(1, **i32)

    def select(name, values, threshold, frustum, final):
        # survivors kept: all of them when the host knows the input's length; else B*N for a list that feeds another stage
        # (4 bytes per node) and max_points for the result
        # (with a band the density survivors are kept whole for the leak count and cut to max_points afterwards)
        capacity = stage.extent if eager else (max_points if final and not (band is not None and name == "density") else total)
        out_idx = torch.empty(max(capacity, 1), **i32)
        out_count = torch.empty(1, **i32)
        hip.field_select(cg, b, stage.extent, out_idx, out_count, values=values, threshold=float(threshold),
                         cams=cams if frustum else None, indices=stage.indices, count=stage.count)
        counts.append(out_count)
        names.append(name)
        stage.indices, stage.count = out_idx, out_count
        if eager:
            stage.extent, stage.count = int(out_count.item()), None
        else:
            stage.extent = capacity

    if in_frustum:
        select("frustum", None, 0.0, True, False)
    if cull is not None and stage.extent > 0:
        net = model.proposal_networks[proposal_level]
        w, bias = net.packed()
        gmap, base = _map_of(net, feats)
        values = torch.empty(stage.extent, **f32)
        hip.field_forward(cg, stage.indices, stage.count, stage.extent, cams, hip.make_feature_map(gmap), base, base, 0, w, bias,
                          density=values, precision=net.precision)
        select("proposal", values, cull, False, False)
    w, bd, bc, bj = dec.packed()
    if is_flow:   # (its own hoisted_map adds the per-image action bias of the flow head, which is not evaluated here)
        gmap, base = ActionDecoderJacobian.hoisted_map(dec, feats), 0
    else:
        gmap, base = _map_of(dec, feats)
    fmap = hip.make_feature_map(gmap)
    common = dict(goff_density=base + dec.GOFF_DENSITY, goff_jacobian=base + dec.GOFF_JACOBIAN, mode=1, w_all=w, b_density=bd,
                  precision=dec.precision)
    if stage.extent > 0:
        values = torch.empty(stage.extent, **f32)
        hip.field_forward(cg, stage.indices, stage.count, stage.extent, cams, fmap, density=values, **common)
        select("density", values, density_threshold, False, not filtering)
        if band is not None:
            if stage.extent > 0:
                leaks = _leaks(grid, band.band, stage.indices, stage.count, stage.extent)
            if not eager and not filtering:
                stage.indices, stage.extent = _rows(stage.indices, max_points), max_points
    else:
        stage.indices, stage.count = torch.empty(0, **i32), None
        counts.append(torch.zeros(1, **i32))
        names.append("density")
    components_status = None
    if filtering and stage.extent > 0:
        flags, components_status = _component_flags(grid, b, stage.indices, stage.count, stage.extent, connectivity,
                                                    min_component_nodes, bool(largest_only), eager)
        select("components", flags, 0.5, False, True)
    elif filtering:
        counts.append(torch.zeros(1, **i32))
        names.append("components")
    n = stage.extent
    a_dim = dec.kernel_action_dim
    index = stage.indices[:n]
    cloud = FieldPointCloud(grid=grid, index=index, xyz=torch.empty(n, 3, **f32), density=torch.empty(n, **f32),
                            color=torch.empty(n, 3, **f32) if want_color else None,
                            jacobian=torch.empty(n, a_dim, 3, **f32) if want_jacobian else None,
                            count=counts[-1], stage_counts=tuple(counts), stage_names=tuple(names))
    if n > 0:
        hip.field_points(cg, b, index, stage.count, n, cloud.xyz)
        if want_color or want_jacobian:
            # the density network runs again on the survivors: cheaper than the Jacobian head on what the selection rejects
            hip.field_forward(cg, index, stage.count, n, cams, fmap, b_color=bc, b_jacobian=bj if want_jacobian else None,
                              jacobian_kind=dec.JACOBIAN_KIND if want_jacobian else hip.JACOBIAN_NONE, density=cloud.density,
                              color=cloud.color,
                              jacobian=cloud.jacobian, view_direction=view_direction,
                              jacobian_precision=dec.j_precision if want_jacobian else None, **common)
        else:
            hip.field_forward(cg, index, stage.count, n, cams, fmap, density=cloud.density, **common)
    if components_status is not None:
        cloud.components_status = components_status
    if band is not None:
        cloud.band_count, cloud.band_leaks = band.count, leaks
    return cloud


# ---- one field per multi-camera scene -------------------------------------------------------------------
def _check_fusion_arguments(name: str, batch: int, views_per_scene, mode, min_views) -> None:
    if isinstance(views_per_scene, bool) or not isinstance(views_per_scene, int) or views_per_scene < 1:
        raise ValueError(f"{name}: views_per_scene must be an integer >= 1 (got {views_per_scene!r})")
    if views_per_scene > hip.FIELD_MAX_VIEWS:
        raise ValueError(f"{name}: at most {hip.FIELD_MAX_VIEWS} views per scene (got {views_per_scene})")
    if batch % views_per_scene != 0:
        raise ValueError(f"{name}: views_per_scene = {views_per_scene} does not divide the batch of {batch} context images")
    if mode not in hip.FIELD_FUSE_MODES:
        raise ValueError(f"{name}: fuse must be one of {sorted(hip.FIELD_FUSE_MODES)} (got {mode!r})")
    if isinstance(min_views, bool) or not isinstance(min_views, int) or not 1 <= min_views <= views_per_scene:
        raise ValueError(f"{name}: min_views must be an integer in [1, views_per_scene = {views_per_scene}] (got {min_views!r})")


def _fuse(grid: FieldGrid, values: torch.Tensor, cams, views: int, mode: str, min_views: int):
    """values [B, N] -> (fused [G, N] fp32, seen [G, N] uint8, valid [G, N] bool): one launch."""
    scenes, dev = values.shape[0] // views, values.device
    fused = torch.empty(scenes, grid.num_nodes, dtype=torch.float32, device=dev)
    seen = torch.empty(scenes, grid.num_nodes, dtype=torch.uint8, device=dev)
    valid = torch.empty(scenes, grid.num_nodes, dtype=torch.bool, device=dev)
    hip.field_fuse(grid.c_grid(), scenes, views, values.reshape(-1), hip.FIELD_FUSE_MODES[mode], min_views, fused, seen, valid,
                   cams=cams)
    return fused, seen, valid


def fuse_views(grid: FieldGrid, values: torch.Tensor, pixel_encoding: Optional[PixelEncoding] = None, *, views_per_scene: int,
               mode: str = "mean", min_views: int = 1):
    """Fuse any per-view scalar on the grid, without the networks: ``values`` ``[B, N]`` fp32 on the GPU, the B batch elements
    being B / V scenes of V = ``views_per_scene`` consecutive views.  Returns ``(fused [G, N] fp32, seen [G, N] uint8, valid
    [G, N] bool)``: bit v of ``seen`` says that view v of the scene holds the node in its frustum (the predicate of the
    selection on the cameras of ``pixel_encoding``; every view sees every node without one), a node is ``valid`` when at least
    ``min_views`` views see it, and ``fused`` is the ``mode`` ("mean", "min" -- carving --, "max") of the values of the views
    that see a valid node, 0 at an invalid one.  ``mesh_from_values(grid, fused, threshold, valid=valid)`` meshes the result."""
    if not torch.is_tensor(values) or values.dim() != 2 or values.dtype != torch.float32 or values.shape[1] != grid.num_nodes:
        raise ValueError(f"fuse_views: values must be fp32 [B, {grid.num_nodes}]")
    _check_fusion_arguments("fuse_views", values.shape[0], views_per_scene, mode, min_views)
    if values.shape[0] < 1 or values.shape[0] * grid.num_nodes >= 2 ** 31:
        raise ValueError("fuse_views: batch * nx*ny*nz must stay below 2**31")
    if pixel_encoding is not None and pixel_encoding.extrinsics.shape[0] != values.shape[0]:
        raise ValueError(f"fuse_views: {pixel_encoding.extrinsics.shape[0]} cameras for {values.shape[0]} rows of values")
    if values.device.type != "cuda":
        raise ValueError("fuse_views: values must live on the GPU; there is no CPU path")
    cams = None if pixel_encoding is None else _cameras(pixel_encoding, False, action_dim=None)
    return _fuse(grid, values.contiguous(), cams, views_per_scene, mode, min_views)


def _decoder_arguments(model, feats):
    """(feature map, density / Jacobian offsets into it, packed weights and biases) of the decoder on ``feats``."""
    dec = model.decoder
    w, bd, bc, bj = dec.packed()
    if isinstance(dec, ActionDecoderFlowMlp):
        gmap, base = ActionDecoderJacobian.hoisted_map(dec, feats), 0
    else:
        gmap, base = _map_of(dec, feats)
    goffs = dict(goff_density=base + dec.GOFF_DENSITY, goff_jacobian=base + dec.GOFF_JACOBIAN)
    return hip.make_feature_map(gmap), goffs, w, bd, bc, bj


def _per_view(node: torch.Tensor, count: Optional[torch.Tensor], nodes: int, views: int):
    """Fused global indices ``g*N + n`` [n] -> the per-view global indices ``(g*V + v)*N + n`` [n*V], entry-major (row
    ``i*V + v``), and the device count times V.  Integer index arithmetic; rows past the count hold whatever the list held
    (the kernels clamp indices and never read past the count)."""
    g = torch.div(node, nodes, rounding_mode="floor")
    base = node + g * ((views - 1) * nodes)                                     # (g*V)*N + n
    step = torch.arange(views, dtype=torch.int32, device=node.device) * nodes
    return (base[:, None] + step[None, :]).reshape(-1), None if count is None else count * views


def _combine(dec, xyz, node, count, n, nodes, views, cams, rows, want_color, want_jacobian):
    """The combine launch on the per-view ``rows`` = (density, color, jacobian) -> (color, jacobian, views) of the n entries."""
    dev = xyz.device
    f32 = dict(dtype=torch.float32, device=dev)
    a_dim = dec.kernel_action_dim
    color = torch.empty(n, 3, **f32) if want_color else None
    jacobian = torch.empty(n, a_dim, 3, **f32) if want_jacobian else None
    seen = torch.empty(n, dtype=torch.uint8, device=dev)
    if n > 0:
        hip.field_combine(xyz, node, count, n, nodes, views, cams, rows[0], color=rows[1], jacobian=rows[2],
                          action_dim=a_dim if want_jacobian else 0, out_color=color, out_jacobian=jacobian, out_views=seen)
    return color, jacobian, seen


def _per_view_rows(dec, n, views, want_color, want_jacobian, dev):
    f32 = dict(dtype=torch.float32, device=dev)
    if not (want_color or want_jacobian):
        return None, None, None
    return (torch.empty(n * views, **f32), torch.empty(n * views, 3, **f32) if want_color else None,
            torch.empty(n * views, 3 * dec.kernel_action_dim, **f32) if want_jacobian else None)


def _extract_field_fused(model, enc, grid, threshold, cams, in_frustum, view_direction, want_color, want_jacobian, max_points,
                         views, mode, min_views, components=None, coarse=None) -> FieldPointCloud:
    """extract_field for scenes of ``views`` views: dense per-view density pass, fuse, ordered selection on the fused values,
    coordinates, the decoder on the survivors of every view, combine.  One host read (the survivor count) without
    ``max_points``, none with it."""
    dec = model.decoder
    dev = enc.features.device
    b, nodes = enc.extrinsics.shape[0], grid.num_nodes
    scenes = b // views
    cg = grid.c_grid()
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    fmap, goffs, w, bd, bc, bj = _decoder_arguments(model, enc.features)
    common = dict(mode=1, w_all=w, b_density=bd, precision=dec.precision, **goffs)
    band = None
    if coarse is None:
        values = torch.empty(b, nodes, **f32)
        hip.field_forward(cg, None, None, b * nodes, cams, fmap, density=values.reshape(-1), **common)
    else:
        band = _extraction_band(model, enc, grid, cams, coarse[0], coarse[1], coarse[2], max_points is None, views, mode,
                                min_views, in_frustum)
        values, _ = _banded_values(model, enc, grid, cams, band, in_frustum, max_points is None, views)
    fused, _, valid = _fuse(grid, values, cams if in_frustum else None, views, mode, min_views)
    del values
    if band is not None:
        valid = valid & band.band.to(torch.bool)
    # an invalid node (fused = 0) must not pass a threshold <= 0: -inf in its place, in the buffer nothing else reads
    fused.masked_fill_(~valid, -math.inf)
    # (with a component filter behind it the density selection keeps every survivor: a truncated list would cut components;
    # so would it the leak count of a band)
    whole = max_points is None or components is not None or band is not None
    capacity = scenes * nodes if whole else max_points
    index, count = torch.empty(max(capacity, 1), **i32), torch.empty(1, **i32)
    hip.field_select(cg, scenes, scenes * nodes, index, count, values=fused.reshape(-1), threshold=threshold)
    leaks = None if band is None else _leaks(grid, band.band, index, count, capacity)
    if band is not None and components is None and max_points is not None:
        index, capacity = _rows(index, max_points), max_points
    n, dev_count = (int(count.item()), None) if max_points is None else (capacity, count)
    index = index[:n]
    stage_counts, stage_names, components_status = (count,), ("density",), None
    if band is not None:
        stage_counts, stage_names = (band.count,) + stage_counts, ("band",) + stage_names
    if components is not None:
        kept, count = torch.empty(max(n if max_points is None else max_points, 1), **i32), torch.empty(1, **i32)
        if n > 0:
            flags, components_status = _component_flags(grid, scenes, index, dev_count, n, components[0], components[1],
                                                        components[2], max_points is None)
            hip.field_select(cg, scenes, n, kept, count, values=flags, threshold=0.5, indices=index, count=dev_count)
        else:
            count.zero_()
        n, dev_count = (int(count.item()), None) if max_points is None else (max_points, count)
        index = kept[:n]
        stage_counts, stage_names = stage_counts + (count,), stage_names + ("components",)
    # (padded rows of a capacity form hold no index: clamped, so the gather stays inside the buffer)
    at = index.long() if dev_count is None else index.clamp(0, scenes * nodes - 1).long()
    cloud = FieldPointCloud(grid=grid, index=index, xyz=torch.empty(n, 3, **f32), density=fused.reshape(-1)[at], color=None,
                            jacobian=None, count=count, stage_counts=stage_counts, stage_names=stage_names)
    if components_status is not None:
        cloud.components_status = components_status
    if band is not None:
        cloud.band_count, cloud.band_leaks = band.count, leaks
    if n > 0:
        hip.field_points(cg, scenes, index, dev_count, n, cloud.xyz)
    rows = _per_view_rows(dec, n, views, want_color, want_jacobian, dev)
    if n > 0 and rows[0] is not None:
        expanded, expanded_count = _per_view(index, dev_count, nodes, views)
        hip.field_forward(cg, expanded, expanded_count, n * views, cams, fmap, b_color=bc, b_jacobian=bj if want_jacobian else None,
                          jacobian_kind=dec.JACOBIAN_KIND if want_jacobian else hip.JACOBIAN_NONE, density=rows[0], color=rows[1],
                          jacobian=rows[2], view_direction=view_direction,
                          jacobian_precision=dec.j_precision if want_jacobian else None, **common)
    cloud.color, cloud.jacobian, cloud.views = _combine(dec, cloud.xyz, index, dev_count, n, nodes, views,
                                                        cams if in_frustum else None, rows, want_color, want_jacobian)
    return cloud


# ---- isosurface meshes ------------------------------------------------------------------------------------------------------
@dataclass
class FieldMesh:
    """The isosurface ``values == threshold`` of a scalar on the grid (marching tetrahedra on the Kuhn cut; DESIGN.md section
    11).  Vertices in ascending ``(vertex_node, vertex_edge)``, triangles in ascending ``triangle_cell``; the geometric normal
    of a triangle points from inside (``values >= threshold``) to outside.  Exactly sized from an eager call; padded to the
    capacities from a capture-safe one, where ``vertex_count`` / ``triangle_count`` hold the TRUE numbers -- they may exceed
    the rows stored, which are the first ones -- and triangle entries are TRUE vertex ranks (check ``vertex_count <=
    max_vertices`` before indexing with them).  A vertex is referenced by at least one triangle unless ``valid`` (or the
    frustum) removed every tetrahedron around its edge."""

    grid: FieldGrid
    vertices: torch.Tensor                # [V, 3]
    vertex_node: torch.Tensor             # [V] int32 global index of the node that owns the vertex's edge
    vertex_edge: torch.Tensor             # [V] uint8 direction 0..6 of the edge (MESH_DIRECTIONS)
    vertex_t: torch.Tensor                # [V] position on the edge: vertices = fma(t, x1 - x0, x0)
    triangles: torch.Tensor               # [T, 3] int32 vertex ranks
    triangle_cell: torch.Tensor           # [T] int32 global cell index
    color: Optional[torch.Tensor]         # [V, 3]
    jacobian: Optional[torch.Tensor]      # [V, A, 3]
    vertex_count: torch.Tensor            # [1] int32
    triangle_count: torch.Tensor          # [1] int32
    vertex_views: Optional[torch.Tensor] = None   # [V] uint8, fused extraction only: bit v = view v sees the vertex position

    @property
    def batch_index(self) -> torch.Tensor:
        """Batch element of every vertex."""
        return torch.div(self.vertex_node, self.grid.num_nodes, rounding_mode="floor")

    def valid(self) -> Tuple[int, int]:
        """(vertex rows, triangle rows) that hold data (reads both counts: a host synchronisation)."""
        return (min(int(self.vertex_count.item()), self.vertex_node.shape[0]),
                min(int(self.triangle_count.item()), self.triangle_cell.shape[0]))

    def colors(self, color_map, mode: int = 0) -> torch.Tensor:
        """``[V, 3]`` display colours in [0, 1] of the valid vertices: ``FieldPointCloud.colors`` on the vertex Jacobians."""
        return _sensitivity_colors("FieldMesh", self.jacobian, self.valid()[0], color_map, mode)

    def save_ply(self, path, colors: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """Binary little-endian PLY: vertices ``x y z`` float32 + ``red green blue`` uint8 (``colors`` ``[V, 3]`` in [0, 1];
        default: the colour head's output, white without one), faces ``list uchar int vertex_indices``.  Returns (V, T)."""
        v, t = self.valid()
        if int(self.vertex_count.item()) > v:
            raise ValueError("save_ply: the mesh was truncated (vertex_count > max_vertices): its triangles reference rows "
                             "that were not stored")
        rgb8 = _rgb8("save_ply", colors, self.color, v)
        vertex = np.empty(v, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
        xyz = self.vertices[:v].detach().cpu().numpy()
        vertex["x"], vertex["y"], vertex["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        vertex["red"], vertex["green"], vertex["blue"] = rgb8[:, 0], rgb8[:, 1], rgb8[:, 2]
        face = np.empty(t, dtype=[("n", "u1"), ("v", "<i4", (3,))])
        face["n"] = 3
        face["v"] = self.triangles[:t].detach().cpu().numpy()
        header = ("ply\nformat binary_little_endian 1.0\ncomment Jacobian-field surface mesh\n"
                  f"element vertex {v}\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                  f"element face {t}\nproperty list uchar int vertex_indices\nend_header\n")
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(vertex.tobytes())
            f.write(face.tobytes())
        return v, t


MESH_DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))   # edge k = lower node + this


def _check_mesh_arguments(name: str, grid: FieldGrid, batch: int, threshold: float, max_vertices, max_triangles) -> None:
    if any(d < 2 for d in grid.dims):
        raise ValueError(f"{name}: every grid dimension must be >= 2 (got {grid.dims}): a mesh needs cells")
    if not math.isfinite(float(threshold)):
        raise ValueError(f"{name}: the threshold must be finite")
    if (max_vertices is None) != (max_triangles is None):
        raise ValueError(f"{name}: give both max_vertices and max_triangles (no host synchronisation) or neither")
    if max_vertices is not None and (max_vertices < 1 or max_triangles < 1):
        raise ValueError(f"{name}: max_vertices and max_triangles must be >= 1")
    if batch < 1 or batch * grid.num_nodes >= 2 ** 31:
        raise ValueError(f"{name}: batch * nx*ny*nz must stay below 2**31")


def _mesh_geometry(grid: FieldGrid, values: torch.Tensor, threshold: float, valid, cams, max_vertices, max_triangles) -> FieldMesh:
    """The six meshing launches.  Eager (no capacities): count, read the count, emit exactly -- for vertices, then triangles."""
    b, dev = values.shape[0], values.device
    total = b * grid.num_nodes
    cg = grid.c_grid()
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    mask, offset = torch.empty(total, **u8), torch.empty(total, **i32)
    v_count, t_count = torch.empty(1, **i32), torch.empty(1, **i32)
    flat = values.reshape(-1)

    def vertices(phase, cap, v_ws):
        out = (torch.empty(cap, **i32), torch.empty(cap, **u8), torch.empty(cap, **f32), torch.empty(cap, 3, **f32))
        hip.field_mesh_vertices(cg, b, flat, threshold, phase, mask, offset, v_count, v_ws, valid=valid, cams=cams,
                                vertex_node=out[0] if cap else None, vertex_edge=out[1] if cap else None,
                                vertex_t=out[2] if cap else None, vertices=out[3] if cap else None)
        return out

    def triangles(phase, cap, t_ws):
        out = (torch.empty(cap, 3, **i32), torch.empty(cap, **i32))
        hip.field_mesh_triangles(cg, b, flat, threshold, phase, mask, offset, t_count, t_ws,
                                 triangles=out[0] if cap else None, triangle_cell=out[1] if cap else None)
        return out

    v_ws, t_ws = hip.field_mesh_workspace(total, dev), hip.field_mesh_workspace(total, dev)
    both = hip.FIELD_MESH_COUNT | hip.FIELD_MESH_EMIT
    if max_vertices is not None:
        v_out = vertices(both, max_vertices, v_ws)
        t_out = triangles(both, max_triangles, t_ws)
    else:
        hip.field_mesh_vertices(cg, b, flat, threshold, hip.FIELD_MESH_COUNT, mask, offset, v_count, v_ws, valid=valid, cams=cams)
        v_out = vertices(hip.FIELD_MESH_EMIT, int(v_count.item()), v_ws)
        if v_out[0].shape[0] == 0:                 # no vertex, no triangle
            t_count.zero_()
            t_out = (torch.empty(0, 3, **i32), torch.empty(0, **i32))
        else:
            hip.field_mesh_triangles(cg, b, flat, threshold, hip.FIELD_MESH_COUNT, mask, offset, t_count, t_ws)
            t_out = triangles(hip.FIELD_MESH_EMIT, int(t_count.item()), t_ws)
    return FieldMesh(grid=grid, vertices=v_out[3], vertex_node=v_out[0], vertex_edge=v_out[1], vertex_t=v_out[2],
                     triangles=t_out[0], triangle_cell=t_out[1], color=None, jacobian=None, vertex_count=v_count,
                     triangle_count=t_count)


def mesh_from_values(grid: FieldGrid, values: torch.Tensor, threshold: float, *, valid: Optional[torch.Tensor] = None,
                     max_vertices: Optional[int] = None, max_triangles: Optional[int] = None) -> FieldMesh:
    """The isosurface of any scalar on the grid, geometry only (``color`` and ``jacobian`` are None): ``values`` ``[B, N]`` fp32
    on the GPU, inside where ``values >= threshold`` (NaN is outside); ``valid`` ``[B, N]`` bool / uint8 removes nodes -- no
    vertex on an edge with an invalid end, no triangle from a tetrahedron with an invalid corner, so the surface is open
    there.  Without capacities: exactly sized tensors, two host reads of a device count.  With both: no host
    synchronisation, tensors padded to the capacities, true counts (see ``FieldMesh``)."""
    if not torch.is_tensor(values) or values.dim() != 2 or values.dtype != torch.float32 or values.shape[1] != grid.num_nodes:
        raise ValueError(f"mesh_from_values: values must be fp32 [B, {grid.num_nodes}]")
    _check_mesh_arguments("mesh_from_values", grid, values.shape[0], threshold, max_vertices, max_triangles)
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8) or valid.shape != values.shape:
            raise ValueError(f"mesh_from_values: valid must be bool or uint8 {tuple(values.shape)}")
        if valid.device != values.device:
            raise ValueError("mesh_from_values: valid and values must live on the same device")
        valid = valid.contiguous()
    if values.device.type != "cuda":
        raise ValueError("mesh_from_values: values must live on the GPU; there is no CPU path")
    return _mesh_geometry(grid, values.contiguous(), float(threshold), valid, None, max_vertices, max_triangles)


@torch.no_grad()
def extract_mesh(model, pixel_encoding: PixelEncoding, grid: FieldGrid, density_threshold: float, *, in_frustum: bool = True,
                 want_color: bool = True, want_jacobian: bool = True, view_direction: Optional[Sequence[float]] = None,
                 max_vertices: Optional[int] = None, max_triangles: Optional[int] = None, views_per_scene: int = 1,
                 fuse: str = "mean", min_views: int = 1, min_component_nodes: Optional[int] = None,
                 largest_only: bool = False, coarse: Optional[int] = None, coarse_threshold: Optional[float] = None,
                 coarse_dilate: int = 1) -> FieldMesh:
    """The surface ``decoder_density == density_threshold`` of the context image(s) over ``grid``, with the colour head's
    output and the Jacobian ``[A, 3]`` AT every vertex (what ``njf_points_forward`` returns for that position and batch
    element).  ``in_frustum``: nodes outside the context view are invalid -- the surface ends where the view ends.  The
    density network runs on all ``B*N`` nodes, ``mesh_from_values`` on the result, one ragged launch on the vertices.

    ``views_per_scene=V > 1``: ONE mesh per scene of V consecutive views -- the surface of the ``fuse``d
    density with the nodes that fewer than ``min_views`` views see (``in_frustum``) invalid; ``vertex_node``, the cells and
    ``batch_index`` are in scene space; colour and Jacobian are the density-weighted mean over the views that see the vertex,
    ``vertex_views`` their bitmask.

    ``min_component_nodes=K`` and / or ``largest_only``: the inside nodes are labelled into connected
    components at connectivity 14 -- the mesh's own: the edges of the Kuhn tetrahedra -- and the nodes of the components below
    K nodes (``largest_only``: of all but the largest) become invalid for the mesher, which removes exactly the tetrahedra
    that carry their surface.  The capacity form leaves the labelling's status word in the attribute ``components_status``.

    ``coarse=k`` / ``coarse_threshold`` / ``coarse_dilate`` (see ``extract_field``): the density network
    runs on every k-th node per axis and then on the band around the coarse hits only, instead of on all ``B*N`` nodes; the mesh
    is that of the same call without ``coarse`` with the nodes outside the band invalid -- identical wherever the band holds
    the surface, which ``band_leaks == 0`` (an attribute of the result, int32 ``[1]``, next to ``band_count``) proves for every
    body the band touches.  Lower ``coarse_threshold`` (default: ``density_threshold``) for parts thinner than k nodes."""
    dec = model.decoder
    if not isinstance(dec, ActionDecoderJacobian):
        raise TypeError("extract_mesh needs one of the fused action decoders")
    _check_fusion_arguments("extract_mesh", pixel_encoding.extrinsics.shape[0], views_per_scene, fuse, min_views)
    _check_component_arguments("extract_mesh", 14, min_component_nodes)
    coarse_threshold = _check_band_arguments("extract_mesh", grid, coarse, coarse_threshold, coarse_dilate, density_threshold)
    components = (min_component_nodes, bool(largest_only)) if min_component_nodes is not None or largest_only else None
    is_flow = isinstance(dec, ActionDecoderFlowMlp)
    if want_jacobian and is_flow:
        raise NotImplementedError("flow_mlp predicts the scene flow directly; it has no Jacobian")
    if view_direction is not None and len(view_direction) != 3:
        raise ValueError("extract_mesh: view_direction has three components")
    feats = pixel_encoding.features
    dev = feats.device
    b = pixel_encoding.extrinsics.shape[0]
    _check_mesh_arguments("extract_mesh", grid, b, density_threshold, max_vertices, max_triangles)
    total = b * grid.num_nodes
    cg = grid.c_grid()
    if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        model.reset_image_cache()      # a capture must contain the projection (see extract_field)
    f32 = dict(dtype=torch.float32, device=dev)
    cams = _cameras(pixel_encoding, False, action_dim=dec.kernel_action_dim if want_jacobian else None)
    if views_per_scene > 1:
        return _extract_mesh_fused(model, pixel_encoding, grid, float(density_threshold), cams, in_frustum, view_direction,
                                   want_color, want_jacobian, max_vertices, max_triangles, views_per_scene, fuse, min_views,
                                   components, None if coarse is None else (coarse, coarse_threshold, coarse_dilate))
    w, bd, bc, bj = dec.packed()
    if is_flow:
        gmap, base = ActionDecoderJacobian.hoisted_map(dec, feats), 0
    else:
        gmap, base = _map_of(dec, feats)
    fmap = hip.make_feature_map(gmap)
    goffs = dict(goff_density=base + dec.GOFF_DENSITY, goff_jacobian=base + dec.GOFF_JACOBIAN)
    band = None
    if coarse is None:
        values = torch.empty(b, grid.num_nodes, **f32)
        hip.field_forward(cg, None, None, total, cams, fmap, mode=1, w_all=w, b_density=bd, density=values.reshape(-1),
                          precision=dec.precision, **goffs)
    else:
        band = _extraction_band(model, pixel_encoding, grid, cams, coarse, coarse_threshold, coarse_dilate, max_vertices is None)
        values, on_list = _banded_values(model, pixel_encoding, grid, cams, band, in_frustum, max_vertices is None)
    keep, components_status = _mesh_keep(grid, values, float(density_threshold), None if band is None else band.band,
                                         cams if in_frustum else None, components, max_vertices is None)
    mesh = _mesh_geometry(grid, values, float(density_threshold), keep, cams if in_frustum else None, max_vertices,
                          max_triangles)
    if components_status is not None:
        mesh.components_status = components_status
    if band is not None:
        # the inside nodes: the list the density ran on (the band, in the view) selected by its compact values
        mesh.band_count = band.count
        mesh.band_leaks = _inside_leaks(grid, b, band, on_list[3], float(density_threshold), *on_list[:3])
    n = mesh.vertex_node.shape[0]
    if want_color:
        mesh.color = torch.empty(n, 3, **f32)
    if want_jacobian:
        mesh.jacobian = torch.empty(n, dec.kernel_action_dim, 3, **f32)
    if n > 0 and (want_color or want_jacobian):
        hip.field_forward_at(mesh.vertices, mesh.vertex_node, None if max_vertices is None else mesh.vertex_count, n,
                             grid.num_nodes, cams, fmap, w_all=w, b_density=bd, b_color=bc,
                             b_jacobian=bj if want_jacobian else None,
                             jacobian_kind=dec.JACOBIAN_KIND if want_jacobian else hip.JACOBIAN_NONE, color=mesh.color,
                             jacobian=mesh.jacobian, view_direction=view_direction, precision=dec.precision,
                             jacobian_precision=dec.j_precision if want_jacobian else None, **goffs)
    return mesh


def _mesh_keep(grid: FieldGrid, values: torch.Tensor, threshold: float, valid, cams, components, eager: bool):
    """(``valid & ~dropped`` for the mesher, status word) of the component filter ``components`` = (min nodes, largest only) on
    the dense values; (``valid``, None) without one.  The labelling sees the mesher's own inside and valid predicates."""
    if components is None:
        return valid, None
    comp = _components(grid, values.shape[0], 14, values.device, values=values.reshape(-1), threshold=threshold, valid=valid,
                       cams=cams)
    if eager:
        _raise_on_status("extract_mesh", comp.status)
    # the mesher's mask: valid and not an inside node of a dropped component (an outside node keeps its validity -- `keep` is
    # false on it by definition, and the surface of a kept component is made of edges that end on outside nodes)
    inside_dropped = (comp.labels >= 0) & ~comp.keep(1 if components[0] is None else components[0], components[1])
    keep = ~inside_dropped if valid is None else valid.to(torch.bool) & ~inside_dropped
    return keep.contiguous(), comp.status


def _extract_mesh_fused(model, enc, grid, threshold, cams, in_frustum, view_direction, want_color, want_jacobian, max_vertices,
                        max_triangles, views, mode, min_views, components=None, coarse=None) -> FieldMesh:
    """extract_mesh for scenes of ``views`` views: dense per-view density pass, fuse, the six meshing launches on the fused
    values with ``valid``, the decoder at every vertex for every view, combine."""
    dec = model.decoder
    dev = enc.features.device
    b, nodes = enc.extrinsics.shape[0], grid.num_nodes
    f32 = dict(dtype=torch.float32, device=dev)
    fmap, goffs, w, bd, bc, bj = _decoder_arguments(model, enc.features)
    band, leaks = None, None
    if coarse is None:
        values = torch.empty(b, nodes, **f32)
        hip.field_forward(grid.c_grid(), None, None, b * nodes, cams, fmap, mode=1, w_all=w, b_density=bd,
                          density=values.reshape(-1), precision=dec.precision, **goffs)
    else:
        band = _extraction_band(model, enc, grid, cams, coarse[0], coarse[1], coarse[2], max_vertices is None, views, mode,
                                min_views, in_frustum)
        values, _ = _banded_values(model, enc, grid, cams, band, in_frustum, max_vertices is None, views)
    fused, _, valid = _fuse(grid, values, cams if in_frustum else None, views, mode, min_views)
    del values
    if band is not None:
        valid = valid & band.band.to(torch.bool)
        leaks = _inside_leaks(grid, b // views, band, fused.masked_fill(~valid, -math.inf), threshold)
    valid, components_status = _mesh_keep(grid, fused, threshold, valid, None, components, max_vertices is None)
    mesh = _mesh_geometry(grid, fused, threshold, valid, None, max_vertices, max_triangles)
    if components_status is not None:
        mesh.components_status = components_status
    if band is not None:
        mesh.band_count, mesh.band_leaks = band.count, leaks
    n = mesh.vertex_node.shape[0]
    dev_count = None if max_vertices is None else mesh.vertex_count
    rows = _per_view_rows(dec, n, views, want_color, want_jacobian, dev)
    if n > 0 and rows[0] is not None:
        expanded, expanded_count = _per_view(mesh.vertex_node, dev_count, nodes, views)
        xyz = mesh.vertices[:, None, :].expand(n, views, 3).reshape(n * views, 3)
        hip.field_forward_at(xyz, expanded, expanded_count, n * views, nodes, cams, fmap, w_all=w, b_density=bd, b_color=bc,
                             b_jacobian=bj if want_jacobian else None,
                             jacobian_kind=dec.JACOBIAN_KIND if want_jacobian else hip.JACOBIAN_NONE, density=rows[0],
                             color=rows[1], jacobian=rows[2], view_direction=view_direction, precision=dec.precision,
                             jacobian_precision=dec.j_precision if want_jacobian else None, **goffs)
    mesh.color, mesh.jacobian, mesh.vertex_views = _combine(dec, mesh.vertices, mesh.vertex_node, dev_count, n, nodes, views,
                                                            cams if in_frustum else None, rows, want_color, want_jacobian)
    return mesh
