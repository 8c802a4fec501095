"""Host-side tests of the isosurface extraction: the numpy restatement of the semantics (tests/field_mesh_restatement.py)
against properties that do not depend on it being "right" in any other sense -- closed, consistently oriented surfaces of
known topology -- the per-vertex interpolation bound, ordering, the PLY writer, argument checks and the C ABI's symbols."""
import os
import re

import numpy as np
import pytest
import torch

import field_mesh_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_SYMBOLS = ("njf_field_mesh_vertices", "njf_field_mesh_triangles", "njf_field_forward_at")
DIMS = (12, 11, 10)
ORIGIN = (-1.0, -1.0, -1.0)
STEP = (2.0 / 11, 2.0 / 10, 2.0 / 9)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


@pytest.fixture(scope="module")
def points():
    return R.grid_points(ORIGIN, STEP, DIMS)


def _mesh(values, threshold=0.0, valid=None, dims=DIMS):
    values = np.asarray(values, dtype=np.float32)
    return R.mesh(ORIGIN, STEP, dims, values.reshape(-1, dims[0] * dims[1] * dims[2]), threshold, valid)


# ---- closed surfaces ------------------------------------------------------------------------------------------------------
def test_sphere_is_closed_oriented_and_of_genus_zero(points):
    m = _mesh(R.sphere_field(points, (0.03, -0.02, 0.05), 0.7))
    R.assert_closed_oriented(m["vertices"], m["triangles"], 2)
    # (a faceted sphere: the volume is below the ball's and within the grid step of it)
    assert 0.85 < R.signed_volume(m["vertices"], m["triangles"]) / (4.0 / 3.0 * np.pi * 0.7 ** 3) < 1.0


def test_torus_has_euler_characteristic_zero(points):
    m = _mesh(R.torus_field(points, (0.03, -0.02, 0.05), 0.55, 0.25))
    R.assert_closed_oriented(m["vertices"], m["triangles"], 0)


def test_two_disjoint_spheres_have_euler_characteristic_four(points):
    a = R.sphere_field(points, (-0.45, -0.05, 0.0), 0.33)
    b = R.sphere_field(points, (0.47, 0.05, 0.02), 0.3)
    m = _mesh(np.maximum(a, b))
    R.assert_closed_oriented(m["vertices"], m["triangles"], 4)


def test_batch_elements_are_meshed_independently(points):
    a, b = R.sphere_field(points, (0.03, -0.02, 0.05), 0.7), R.torus_field(points, (0.03, -0.02, 0.05), 0.55, 0.25)
    both, one, two = _mesh(np.stack([a, b])), _mesh(a), _mesh(b)
    n, cells = np.prod(DIMS), np.prod([d - 1 for d in DIMS])
    v = one["vertex_node"].shape[0]
    assert np.array_equal(both["vertex_node"], np.concatenate([one["vertex_node"], two["vertex_node"] + n]))
    assert np.array_equal(both["triangles"], np.concatenate([one["triangles"], two["triangles"] + v]))
    assert np.array_equal(both["triangle_cell"], np.concatenate([one["triangle_cell"], two["triangle_cell"] + cells]))
    assert np.array_equal(both["vertices"], np.concatenate([one["vertices"], two["vertices"]]))


# ---- every vertex -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.0, 0.2])
def test_every_vertex_sits_on_a_crossing_edge_at_the_threshold(points, threshold):
    values = R.smooth_random_field(points, seed=3)
    m = _mesh(values, threshold)
    nx, ny, nz = DIMS
    node = m["vertex_node"].astype(np.int64)
    step = np.array(R.DIRECTIONS)[m["vertex_edge"]]
    index = np.stack([node // (ny * nz), (node // nz) % ny, node % nz], -1)
    assert m["vertex_edge"].max() <= 6 and ((index + step) < np.array(DIMS)).all(), "an edge leaves the grid"
    v0 = values[node]
    v1 = values[node + step[:, 0] * ny * nz + step[:, 1] * nz + step[:, 2]]
    thr = np.float32(threshold)
    assert ((v0 >= thr) != (v1 >= thr)).all()
    t = m["vertex_t"].astype(np.float64)
    assert (t >= 0).all() and (t <= 1).all()
    # one division, one product, one sum: 8 ulps of the largest operand cover it
    residual = np.abs(v0.astype(np.float64) + t * (v1.astype(np.float64) - v0.astype(np.float64)) - np.float64(thr))
    scale = np.maximum(np.maximum(np.abs(v0), np.abs(v1)), np.abs(thr)).astype(np.float32)
    assert (residual <= 8 * np.spacing(scale).astype(np.float64)).all(), float((residual / np.spacing(scale)).max())
    # positions: on the segment between the two node coordinates
    x0 = R.node_coordinates(ORIGIN, STEP, index).astype(np.float64)
    x1 = R.node_coordinates(ORIGIN, STEP, index + step).astype(np.float64)
    assert np.allclose(m["vertices"], x0 + t[:, None] * (x1 - x0), rtol=0, atol=1e-6)


def test_order_of_vertices_and_triangles(points):
    m = _mesh(np.stack([R.smooth_random_field(points, seed=3), R.smooth_random_field(points, seed=4)]))
    key = m["vertex_node"].astype(np.int64) * 8 + m["vertex_edge"]
    assert (np.diff(key) > 0).all(), "vertices are not strictly ascending in (owner, k)"
    assert (np.diff(m["triangle_cell"].astype(np.int64)) >= 0).all()
    assert np.bincount(m["triangle_cell"]).max() <= 12
    assert m["triangles"].min() >= 0 and m["triangles"].max() < key.shape[0]
    assert np.unique(m["triangles"]).size == key.shape[0], "without a mask every vertex is referenced"


# ---- edge cases ---------------------------------------------------------------------------------------------------------------
def test_a_node_exactly_at_the_threshold_is_inside_and_the_surface_stays_closed(points):
    values = R.sphere_field(points, (0.03, -0.02, 0.05), 0.7)
    outside = np.nonzero(values < 0)[0]
    hit = outside[np.argmax(values[outside])]                  # the outside node nearest to the surface moves onto it
    values[hit] = 0.0
    m = _mesh(values)
    R.assert_closed_oriented(m["vertices"], m["triangles"], 2)
    # it is inside: its crossing edges carry vertices ON the node -- t = 0 where it owns the edge, t = 1 where it ends it
    nx, ny, nz = DIMS
    step = np.array(R.DIRECTIONS)[m["vertex_edge"]]
    end = m["vertex_node"] + step[:, 0] * ny * nz + step[:, 1] * nz + step[:, 2]
    owns, ends = m["vertex_node"] == hit, end == hit
    assert owns.sum() + ends.sum() > 0
    assert (m["vertex_t"][owns] == 0.0).all() and (m["vertex_t"][ends] == 1.0).all()


def test_a_nan_node_is_outside(points):
    values = R.sphere_field(points, (0.03, -0.02, 0.05), 0.7)
    hole = int(np.argmax(values))                               # the node nearest to the centre
    values[hole] = np.nan
    m = _mesh(values)
    R.assert_closed_oriented(m["vertices"], m["triangles"], 4)  # the sphere and a small closed cavity around the NaN
    around = m["vertex_node"] == hole
    assert around.any() and (m["vertex_t"][around] == 0.5).all(), "t is not finite on an edge with a NaN end: 0.5"
    assert np.isfinite(m["vertices"]).all()


def test_a_mask_that_removes_a_slab_opens_the_surface_along_it(points):
    values = R.sphere_field(points, (0.03, -0.02, 0.05), 0.7)
    nx, ny, nz = DIMS
    ix = np.arange(nx * ny * nz) // (ny * nz)
    valid = (ix != 6)[None]
    m = _mesh(values, valid=valid)
    own_ix = m["vertex_node"] // (ny * nz)
    end_ix = own_ix + np.array(R.DIRECTIONS)[m["vertex_edge"]][:, 0]
    assert not np.any(own_ix == 6) and not np.any(end_ix == 6)
    d = R.directed_edge_counts(m["triangles"])
    assert all(c == 1 for c in d.values())
    boundary = R.boundary_edges(m["triangles"])
    assert boundary, "the surface must be open"
    for u, v in boundary:                                       # both ends of a boundary edge lie in the planes next to the slab
        for w in (u, v):
            assert own_ix[w] == end_ix[w] and own_ix[w] in (5, 7), (w, own_ix[w], end_ix[w])
    # (vertices on edges between the neighbouring planes and nothing else may be unreferenced)
    assert np.unique(m["triangles"]).size == m["vertex_node"].shape[0]


# ---- the host side of the package -------------------------------------------------------------------------------------------
def _field_mesh(m, grid, color=None, jacobian=None):
    from neural_jacobian_field_amd.field_volume import FieldMesh
    tensor = {k: torch.from_numpy(v) for k, v in m.items()}
    return FieldMesh(grid=grid, vertices=tensor["vertices"], vertex_node=tensor["vertex_node"], vertex_edge=tensor["vertex_edge"],
                     vertex_t=tensor["vertex_t"], triangles=tensor["triangles"], triangle_cell=tensor["triangle_cell"], color=color,
                     jacobian=jacobian, vertex_count=torch.tensor([m["vertex_node"].shape[0]], dtype=torch.int32),
                     triangle_count=torch.tensor([m["triangle_cell"].shape[0]], dtype=torch.int32))


def test_ply_round_trip(points, tmp_path):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    grid = FieldGrid(ORIGIN, STEP, DIMS)
    m = _mesh(np.stack([R.sphere_field(points, (0.03, -0.02, 0.05), 0.7)] * 2))
    v, t = m["vertex_node"].shape[0], m["triangle_cell"].shape[0]
    color = torch.rand(v, 3, generator=torch.Generator().manual_seed(0))
    mesh = _field_mesh(m, grid, color=color)
    assert mesh.valid() == (v, t)
    assert torch.equal(mesh.batch_index, torch.from_numpy(m["vertex_node"] // grid.num_nodes))
    assert mesh.save_ply(tmp_path / "mesh.ply") == (v, t)
    raw = open(tmp_path / "mesh.ply", "rb").read()
    cut = raw.index(b"end_header\n") + 11
    header = raw[:cut].decode("ascii").split("\n")
    assert header[:2] == ["ply", "format binary_little_endian 1.0"]
    assert f"element vertex {v}" in header and f"element face {t}" in header
    assert header[header.index(f"element face {t}") + 1] == "property list uchar int vertex_indices"
    assert "property float density" not in header
    vertex = np.frombuffer(raw, dtype=[("xyz", "<f4", (3,)), ("rgb", "u1", (3,))], count=v, offset=cut)
    face = np.frombuffer(raw, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=t, offset=cut + 15 * v)
    assert len(raw) == cut + 15 * v + 13 * t
    assert np.array_equal(vertex["xyz"], m["vertices"])
    assert np.array_equal(vertex["rgb"], np.rint(color.numpy() * 255.0).astype(np.uint8))
    assert (face["n"] == 3).all() and np.array_equal(face["v"], m["triangles"])
    # explicit colours, white without any, and the refusal of a truncated mesh
    mesh.save_ply(tmp_path / "red.ply", colors=torch.tensor([[1.0, 0.0, 0.0]]).expand(v, 3))
    red = np.frombuffer(open(tmp_path / "red.ply", "rb").read(), dtype=[("xyz", "<f4", (3,)), ("rgb", "u1", (3,))], count=v, offset=cut)
    assert (red["rgb"] == np.array([255, 0, 0], dtype=np.uint8)).all()
    with pytest.raises(ValueError, match="colors must be"):
        mesh.save_ply(tmp_path / "bad.ply", colors=torch.zeros(v + 1, 2))
    mesh.vertex_count = torch.tensor([v + 5], dtype=torch.int32)
    with pytest.raises(ValueError, match="truncated"):
        mesh.save_ply(tmp_path / "bad.ply")


def test_mesh_colours_share_the_point_cloud_colouring(points):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud
    grid = FieldGrid(ORIGIN, STEP, DIMS)
    m = _mesh(R.sphere_field(points, (0.03, -0.02, 0.05), 0.7))
    v = m["vertex_node"].shape[0]
    jac = torch.randn(v, 4, 3, generator=torch.Generator().manual_seed(1))
    color_map = torch.rand(3, 4, generator=torch.Generator().manual_seed(2))
    mesh = _field_mesh(m, grid, jacobian=jac)
    cloud = FieldPointCloud(grid=grid, index=torch.from_numpy(m["vertex_node"]), xyz=torch.from_numpy(m["vertices"]),
                            density=torch.zeros(v), color=None, jacobian=jac, count=torch.tensor([v], dtype=torch.int32))
    assert torch.equal(mesh.colors(color_map), cloud.colors(color_map))
    with pytest.raises(ValueError, match=r"color_map must be \[3, 4\]"):
        mesh.colors(torch.rand(3, 5))
    with pytest.raises(ValueError, match="needs the Jacobians"):
        _field_mesh(m, grid).colors(color_map)


def test_api_errors():
    from neural_jacobian_field_amd.field_volume import FieldGrid, mesh_from_values
    grid = FieldGrid(ORIGIN, STEP, DIMS)
    values = torch.zeros(2, grid.num_nodes)
    for dims in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        flat = FieldGrid(ORIGIN, STEP, dims)
        with pytest.raises(ValueError, match="dimension"):
            mesh_from_values(flat, torch.zeros(1, flat.num_nodes), 0.0)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            mesh_from_values(grid, values, bad)
    for wrong in (values[0], values[:, :-1], values.double(), values.reshape(2, *DIMS), values.numpy()):
        with pytest.raises(ValueError, match="values must be"):
            mesh_from_values(grid, wrong, 0.0)
    for wrong in (torch.ones(2, grid.num_nodes), torch.ones(1, grid.num_nodes, dtype=torch.bool), torch.ones(2, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="valid must be"):
            mesh_from_values(grid, values, 0.0, valid=wrong)
    with pytest.raises(ValueError, match="both"):
        mesh_from_values(grid, values, 0.0, max_vertices=10)
    with pytest.raises(ValueError, match="both"):
        mesh_from_values(grid, values, 0.0, max_triangles=10)
    for caps in ((0, 10), (10, 0), (-1, -1)):
        with pytest.raises(ValueError, match=">= 1"):
            mesh_from_values(grid, values, 0.0, max_vertices=caps[0], max_triangles=caps[1])
    big = FieldGrid(ORIGIN, STEP, (1024, 1024, 64))            # 2**26 nodes: 32 batch elements reach 2**31
    with pytest.raises(ValueError, match=r"2\*\*31"):
        mesh_from_values(big, torch.empty(32, big.num_nodes, device="meta"), 0.0)
    with pytest.raises(ValueError, match="no CPU path"):
        mesh_from_values(grid, values, 0.0)


def test_extract_mesh_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import extract_mesh
    with pytest.raises(TypeError, match="fused action decoders"):
        extract_mesh(type("M", (), {"decoder": object()})(), None, None, 0.0)
    from neural_jacobian_field_amd.model import Model
    assert callable(Model.extract_mesh)


def test_mesh_symbols_are_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    for name in MESH_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/njf_hip.h"
        assert name in hip.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes is not None
    assert lib.njf_abi_version() == 20          # the change is additive
    assert int(re.search(r"#define NJF_FIELD_MESH_BLOCK (\d+)", header).group(1)) == hip.FIELD_MESH_BLOCK
    assert int(re.search(r"#define NJF_FIELD_MESH_COUNT (\d+)", header).group(1)) == hip.FIELD_MESH_COUNT
    assert int(re.search(r"#define NJF_FIELD_MESH_EMIT (\d+)", header).group(1)) == hip.FIELD_MESH_EMIT
    # the bound signatures have the header's number of parameters
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in MESH_SYMBOLS:
        params = re.search(name + r"\s*\((.*?)\);", flat, flags=re.S).group(1)
        assert len(params.split(",")) == len(getattr(lib, name).argtypes), name


def test_the_c_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """NJF_E_VALUE for the new error conditions, checked before any launch."""
    import ctypes as C
    from neural_jacobian_field_amd import hip
    e_value = -8                                               # NJF_E_VALUE
    assert b"value" in lib.njf_error_string(e_value)
    fake = C.c_void_p(4096)                                    # never dereferenced: every call below fails its checks
    def vertices(dims, threshold, phase, max_vertices=0):
        return lib.njf_field_mesh_vertices(C.byref(hip.make_field_grid(ORIGIN, STEP, dims)), None, 1, fake, None, threshold, phase,
                                           fake, fake, None, None, None, None, max_vertices, fake, fake, None)
    assert vertices((1, 4, 4), 0.0, 3) == e_value
    assert vertices((4, 4, 4), float("nan"), 3) == e_value
    assert vertices((4, 4, 4), 0.0, 0) == e_value
    assert vertices((4, 4, 4), 0.0, 4) == e_value
    assert vertices((4, 4, 4), 0.0, 3, max_vertices=-1) == e_value
    assert lib.njf_field_mesh_triangles(C.byref(hip.make_field_grid(ORIGIN, STEP, (4, 4, 1))), 1, fake, 0.0, 3, fake, fake, None,
                                        None, 0, fake, fake, None) == e_value
