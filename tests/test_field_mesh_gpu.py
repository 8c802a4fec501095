"""GPU tests of the isosurface extraction (field_volume.mesh_from_values / extract_mesh; njf_field_mesh_vertices /
njf_field_mesh_triangles / njf_field_forward_at).

Geometry is compared with the numpy restatement of the semantics (tests/field_mesh_restatement.py): every integer output
exactly, ``vertex_t`` and ``vertices`` within 1 fp32 ulp of the larger operand (division and fma are correctly rounded on
both sides).  The closed-surface checks run on the GPU output itself and do not depend on the restatement.  Vertex attributes
are compared bit for bit with ``hip.points_forward`` on the returned positions.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import block_offsets_cases as K
import field_mesh_restatement as R

pytestmark = pytest.mark.gpu

IMG = 64
ORIGIN = (-1.0, -0.9, -0.8)
INT_FIELDS = ("vertex_node", "vertex_edge", "triangles", "triangle_cell")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _grid(dims, upper=(1.0, 0.95, 0.9)):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds(ORIGIN, upper, dims)


def _analytic(grid, kind, batch):
    """[B, N] fp32: a different field per batch element."""
    pts = R.grid_points(grid.origin, grid.step, grid.dims)
    rows = []
    for b in range(batch):
        s = 0.04 * b
        if kind == "sphere":
            rows.append(R.sphere_field(pts, (0.03 + s, -0.02, 0.05 - s), 0.62 - s))
        elif kind == "torus":
            rows.append(R.torus_field(pts, (0.02 - s, 0.03, 0.04 + s), 0.5, 0.24 - s))
        else:
            rows.append(R.smooth_random_field(pts, seed=5 + b))
    return np.stack(rows)


def _numpy(mesh):
    v, t = mesh.valid()
    out = {k: getattr(mesh, k)[:(t if k.startswith("tri") else v)].cpu().numpy()
           for k in INT_FIELDS + ("vertex_t", "vertices")}
    out["counts"] = (int(mesh.vertex_count.item()), int(mesh.triangle_count.item()))
    return out


def _assert_equals_restatement(got, grid, values, threshold, valid=None):
    ref = R.mesh(grid.origin, grid.step, grid.dims, values, threshold, valid)
    assert got["counts"] == (ref["vertex_node"].shape[0], ref["triangle_cell"].shape[0])
    for k in INT_FIELDS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    ulps = (R.ulp_distance(got["vertex_t"], ref["vertex_t"]), R.ulp_distance(got["vertices"], ref["vertices"]))
    print("ulp distance (t, position):", ulps, "bit-equal:", np.array_equal(got["vertex_t"], ref["vertex_t"]),
          np.array_equal(got["vertices"], ref["vertices"]))
    assert ulps[0] <= 1.0 and ulps[1] <= 1.0, ulps
    return ref


def _bytes_equal(a, b):
    fa, fb = _numpy(a), _numpy(b)
    return fa["counts"] == fb["counts"] and all(np.array_equal(fa[k], fb[k]) and fa[k].dtype == fb[k].dtype
                                                for k in INT_FIELDS + ("vertex_t", "vertices"))


# ---- 1. mesh_from_values against the restatement -----------------------------------------------------------------------------
# 9x8x7: small, non-cubic, odd; 17x13x11 = 2431 nodes: three counting blocks with a ragged last one; 40^3: tens of blocks
@pytest.mark.parametrize("dims,batch", [((9, 8, 7), 2), ((17, 13, 11), 2), ((40, 40, 40), 1)])
@pytest.mark.parametrize("kind", ["sphere", "torus", "random"])
def test_mesh_from_values_equals_the_restatement(dev, kind, dims, batch):
    from neural_jacobian_field_amd.field_volume import mesh_from_values
    grid = _grid(dims)
    values = _analytic(grid, kind, batch)
    mesh = mesh_from_values(grid, torch.from_numpy(values).to(dev), 0.0)
    assert mesh.color is None and mesh.jacobian is None
    assert mesh.vertex_node.dtype == torch.int32 and mesh.vertex_edge.dtype == torch.uint8 and mesh.triangles.dtype == torch.int32
    got = _numpy(mesh)
    assert got["counts"] == (mesh.vertices.shape[0], mesh.triangles.shape[0]) and got["counts"][1] > 0
    _assert_equals_restatement(got, grid, values, 0.0)
    assert np.array_equal(mesh.batch_index.cpu().numpy(), got["vertex_node"] // grid.num_nodes)
    if kind != "random":        # closed surfaces strictly inside the grid: the checks run on the GPU output itself
        per_body = 2 if kind == "sphere" else 0
        R.assert_closed_oriented(got["vertices"], got["triangles"], per_body * batch)


@pytest.mark.parametrize("dims,batch,kind", K.MESH_CASES)
def test_mesh_past_256_counting_blocks_equals_the_restatement(dev, dims, batch, kind):
    """Both scans of the mesh (nodes -> vertex offsets, cells -> triangle offsets) with two sums per thread of the one-workgroup
    scan: 281 and 269 workgroups at 67 x 66 x 65, 286 and 270 at two elements of 53 x 52 x 53.  The random field has vertices
    in all workgroups but one, the sphere leaves more than fifty empty at either end (tests/test_block_primitives_cpu.py)."""
    from neural_jacobian_field_amd.field_volume import mesh_from_values
    grid = _grid(dims)
    values = _analytic(grid, kind, batch)
    got = _numpy(mesh_from_values(grid, torch.from_numpy(values).to(dev), 0.0))
    ref = _assert_equals_restatement(got, grid, values, 0.0)
    for what, block_of, total in (("vertices", ref["vertex_node"], batch * grid.num_nodes),
                                  ("triangles", ref["triangle_cell"], batch * (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1))):
        blocks = K.workgroups(total, K.MESH_BLOCK)
        filled = np.unique(block_of // K.MESH_BLOCK)
        print(f"{what}: workgroups {blocks}, per {K.per_thread(blocks)}, survivors {block_of.shape[0]}, in {filled.size} workgroups "
              f"({filled[0]} .. {filled[-1]})")
        assert blocks > K.THREADS and block_of.shape[0] > 0


def test_masked_form_and_special_values(dev):
    """A `valid` mask that removes one slab (bool and uint8 give the same bytes), a NaN node, a node exactly at the threshold."""
    from neural_jacobian_field_amd.field_volume import mesh_from_values
    grid = _grid((17, 13, 11))
    values = _analytic(grid, "sphere", 2)
    values[0, grid.linear_index(8, 6, 5)] = np.nan                       # deep inside the first sphere: a hole around it
    thr = 0.25
    values[1, int(np.argmin(np.abs(values[1] - thr)))] = np.float32(thr)   # exactly the threshold: inside
    valid = np.ones((2, grid.num_nodes), dtype=bool)
    ix = grid.unravel(np.arange(grid.num_nodes))[0]
    valid[:, ix == 9] = False
    dvalues = torch.from_numpy(values).to(dev)
    mesh = mesh_from_values(grid, dvalues, thr, valid=torch.from_numpy(valid).to(dev))
    got = _numpy(mesh)
    _assert_equals_restatement(got, grid, values, thr, valid)
    as_u8 = mesh_from_values(grid, dvalues, thr, valid=torch.from_numpy(valid.astype(np.uint8)).to(dev))
    assert _bytes_equal(mesh, as_u8)
    # the surface is open exactly along the removed slab: every boundary edge joins vertices whose edges touch ix = 8 or 10
    boundary = R.boundary_edges(got["triangles"])
    assert boundary
    own_ix = grid.unravel(got["vertex_node"])[0]
    end_ix = own_ix + np.array(R.DIRECTIONS)[got["vertex_edge"]][:, 0]
    for u, v in boundary:
        for w in (u, v):
            assert own_ix[w] in (8, 10) or end_ix[w] in (8, 10), (w, own_ix[w], end_ix[w])
    # no vertex on an edge with an invalid end
    assert not np.any(own_ix == 9) and not np.any(end_ix == 9)


def test_two_calls_give_equal_bytes(dev):
    from neural_jacobian_field_amd.field_volume import mesh_from_values
    grid = _grid((17, 13, 11))
    values = torch.from_numpy(_analytic(grid, "random", 2)).to(dev)
    assert _bytes_equal(mesh_from_values(grid, values, 0.1), mesh_from_values(grid, values, 0.1))


def test_capacity_form_and_capture(dev):
    """Capacities above the counts: the first rows equal the eager result, also from a captured graph replayed after the values
    were refilled.  Capacities below the counts: true counts, the first rows, true vertex ranks in the triangles."""
    from neural_jacobian_field_amd.field_volume import mesh_from_values
    grid = _grid((17, 13, 11))
    first, second = (torch.from_numpy(_analytic(grid, k, 2)).to(dev) for k in ("random", "torus"))
    eager = [_numpy(mesh_from_values(grid, v, 0.0)) for v in (first, second)]
    cap_v, cap_t = (max(e["counts"][i] for e in eager) + 37 for i in (0, 1))

    def check(mesh, ref, rows_v, rows_t):
        assert mesh.vertex_node.shape[0] == rows_v and mesh.triangles.shape[0] == rows_t
        got = _numpy(mesh)
        assert got["counts"] == ref["counts"]
        kv, kt = min(rows_v, ref["counts"][0]), min(rows_t, ref["counts"][1])
        assert mesh.valid() == (kv, kt)
        for k in INT_FIELDS + ("vertex_t", "vertices"):
            rows = kt if k.startswith("tri") else kv
            assert np.array_equal(got[k][:rows], ref[k][:rows]), k

    static = first.clone()
    check(mesh_from_values(grid, static, 0.0, max_vertices=cap_v, max_triangles=cap_t), eager[0], cap_v, cap_t)   # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mesh_from_values(grid, static, 0.0, max_vertices=cap_v, max_triangles=cap_t)
    graph.replay()
    torch.cuda.synchronize()
    check(captured, eager[0], cap_v, cap_t)
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    check(captured, eager[1], cap_v, cap_t)
    assert eager[0]["counts"] != eager[1]["counts"]
    small_v, small_t = eager[0]["counts"][0] - 33, eager[0]["counts"][1] // 2
    check(mesh_from_values(grid, first, 0.0, max_vertices=small_v, max_triangles=small_t), eager[0], small_v, small_t)
    check(mesh_from_values(grid, first, 0.0, max_vertices=1, max_triangles=1), eager[0], 1, 1)


def test_an_empty_surface(dev):
    from neural_jacobian_field_amd.field_volume import mesh_from_values
    grid = _grid((9, 8, 7))
    values = torch.from_numpy(_analytic(grid, "sphere", 2)).to(dev)
    mesh = mesh_from_values(grid, values, 1e30)
    assert mesh.valid() == (0, 0) and tuple(mesh.triangles.shape) == (0, 3) and tuple(mesh.vertices.shape) == (0, 3)
    padded = mesh_from_values(grid, values, 1e30, max_vertices=8, max_triangles=8)
    assert padded.valid() == (0, 0) and tuple(padded.triangles.shape) == (8, 3)


# ---- 2. extract_mesh on the synthetic model --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model
    cache = {}

    def get(kind, adim):
        if (kind, adim) not in cache:
            cfg = model_cfg_from_dict({"action_dim": adim, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                                       "action_decoder": {"name": kind}})
            model = Model(cfg)
            model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes(kind, adim), seed=0), strict=True)
            cache[(kind, adim)] = model.to(dev).eval().requires_grad_(False)
        return cache[(kind, adim)]

    return get


def _scene_grid(dims):
    """In front of the identity context camera (normalised focal 0.8): the near corners project outside the image."""
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), dims)


def _camera_input(batch, dev, seed=0):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.model import CameraInput
    cams = synthetic.synthetic_cameras(batch)
    c2w = cams["ctxt_c2w"].clone()
    if batch > 1:   # the second image looks from another pose: the batch element of a vertex must pick ITS camera
        c2w[1:] = synthetic.general_pose(7, batch - 1, scale=0.05)
    image = 0.03 * torch.rand(batch, 3, IMG, IMG, generator=torch.Generator().manual_seed(11 + seed))
    return CameraInput(input_image=image.to(dev), ctxt_extrinsics=c2w.to(dev), ctxt_intrinsics=cams["ctxt_k_norm"].to(dev),
                       trgt_extrinsics=c2w.to(dev), trgt_intrinsics=cams["ctxt_k_norm"].to(dev))


def _encoding(cam, adim, seed=1):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    b, dev = cam.input_image.shape[0], cam.input_image.device
    return PixelEncoding(features=synthetic.synthetic_features(b, IMG, IMG, seed=seed).to(dev), extrinsics=cam.ctxt_extrinsics,
                         intrinsics=cam.ctxt_intrinsics, action=synthetic.synthetic_action(b, adim).to(dev))


def _dense_density(model, enc, grid):
    """The existing dense route: grid.points() + compute_density -> [B, N]."""
    b = enc.extrinsics.shape[0]
    xyz = grid.points(device=enc.extrinsics.device)
    head, _ = model.compute_density(xyz[None].expand(b, -1, 3).contiguous(), enc)
    return head.density.reshape(b, grid.num_nodes).clone()


def _median_threshold(density):
    """Half-way between the two middle dense values: the surface is not empty and no node sits on the threshold."""
    s = torch.sort(density.reshape(-1).double().cpu()).values
    k = s.numel() // 2
    return float(0.5 * (s[k - 1] + s[k]))


def _points_forward_rows(model, enc, mesh, want_jacobian, view_direction=None):
    """hip.points_forward on the returned vertex positions, per batch element, padded to the largest one -> rows [V, ...]."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import _cameras, _map_of
    dec = model.decoder
    dev = mesh.vertices.device
    b = enc.extrinsics.shape[0]
    which = mesh.batch_index.long()
    counts = torch.bincount(which, minlength=b)
    pad = max(int(counts.max()), 1)
    xyz = torch.zeros(b, pad, 3, device=dev)
    xyz[:, :, 2] = 1.5
    slot = torch.arange(which.numel(), device=dev) - torch.cumsum(counts, 0)[which] + counts[which]   # ascending per element
    xyz[which, slot] = mesh.vertices
    dirs = None
    if view_direction is not None:
        dirs = torch.tensor(view_direction, dtype=torch.float32, device=dev).expand(b, pad, 3).contiguous()
    cams = _cameras(enc, False, action_dim=dec.kernel_action_dim if want_jacobian else None)
    w, bd, bc, bj = dec.packed()
    gmap, base = _map_of(dec, enc.features)
    a_dim = dec.kernel_action_dim
    color = torch.empty(b * pad, 3, device=dev)
    jac = torch.empty(b * pad, 3 * a_dim, device=dev) if want_jacobian else None
    hip.points_forward(xyz, dirs, cams, hip.make_feature_map(gmap), base + dec.GOFF_DENSITY, base + dec.GOFF_JACOBIAN, 1, w, bd,
                       b_color=bc, b_jacobian=bj if want_jacobian else None,
                       jacobian_kind=dec.JACOBIAN_KIND if want_jacobian else hip.JACOBIAN_NONE, color=color, jacobian=jac,
                       precision=dec.precision, jacobian_precision=dec.j_precision if want_jacobian else None)
    rows = which * pad + slot
    return color[rows], None if jac is None else jac[rows].reshape(-1, a_dim, 3)


@pytest.mark.parametrize("dims", [(9, 8, 7), (17, 13, 11)])
@pytest.mark.parametrize("precision", ["f32", None, "f16"])
@pytest.mark.parametrize("kind,adim", [("jacobian_mlp", 8), ("jacobian_transformer", 6)])
def test_extract_mesh_equals_the_dense_route_and_points_forward(models, dev, kind, adim, precision, dims):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import extract_mesh, mesh_from_values
    model = models(kind, adim)
    model.set_precision(hip.DEFAULT_PRECISION if precision is None else precision)
    try:
        grid = _scene_grid(dims)
        enc = _encoding(_camera_input(2, dev), adim)
        density = _dense_density(model, enc, grid)
        thr = _median_threshold(density)
        mesh = extract_mesh(model, enc, grid, thr, in_frustum=False)
        v, t = mesh.valid()
        assert v == mesh.vertices.shape[0] > 0 and t == mesh.triangles.shape[0] > 0
        assert tuple(mesh.color.shape) == (v, 3) and tuple(mesh.jacobian.shape) == (v, adim, 3)
        counts = torch.bincount(mesh.batch_index.long(), minlength=2)
        assert int(counts.min()) > 0 and int(counts[0]) != int(counts[1]), "the batch must be ragged"
        assert _bytes_equal(mesh, mesh_from_values(grid, density, thr)), "geometry differs from the dense route's"
        color, jac = _points_forward_rows(model, enc, mesh, True)
        assert torch.equal(mesh.color, color)
        assert torch.equal(mesh.jacobian, jac)
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


def test_extract_mesh_options_and_capture(models, dev):
    """Colour only, a view direction, the capacity form under capture (replayed on a second image's features), flow_mlp."""
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import extract_mesh
    model = models("jacobian_mlp", 8)
    grid = _scene_grid((9, 8, 7))
    cam = _camera_input(2, dev)
    enc = _encoding(cam, 8)
    thr = _median_threshold(_dense_density(model, enc, grid))
    full = extract_mesh(model, enc, grid, thr, in_frustum=False)
    direction = (0.6, -0.48, 0.64)
    bare = extract_mesh(model, enc, grid, thr, in_frustum=False, want_jacobian=False, view_direction=direction)
    assert bare.jacobian is None and _bytes_equal(bare, full) and not torch.equal(bare.color, full.color)
    color, _ = _points_forward_rows(model, enc, bare, False, view_direction=direction)
    assert torch.equal(bare.color, color)
    no_color = extract_mesh(model, enc, grid, thr, in_frustum=False, want_color=False)
    assert no_color.color is None and torch.equal(no_color.jacobian, full.jacobian)
    geometry = extract_mesh(model, enc, grid, thr, in_frustum=False, want_color=False, want_jacobian=False)
    assert geometry.color is None and geometry.jacobian is None and _bytes_equal(geometry, full)

    enc2 = PixelEncoding(features=synthetic.synthetic_features(2, IMG, IMG, seed=9).to(dev), extrinsics=enc.extrinsics,
                         intrinsics=enc.intrinsics, action=None)
    eager2 = extract_mesh(model, enc2, grid, thr, in_frustum=True)
    cap_v = max(full.vertices.shape[0], eager2.vertices.shape[0]) + 50
    cap_t = max(full.triangles.shape[0], eager2.triangles.shape[0]) + 50
    static = PixelEncoding(features=enc.features.clone(), extrinsics=enc.extrinsics, intrinsics=enc.intrinsics, action=None)
    kw = dict(in_frustum=True, max_vertices=cap_v, max_triangles=cap_t)
    extract_mesh(model, static, grid, thr, **kw)                   # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = extract_mesh(model, static, grid, thr, **kw)
    static.features.copy_(enc2.features)
    graph.replay()
    torch.cuda.synchronize()
    v, t = captured.valid()
    assert (v, t) == eager2.valid() and captured.vertices.shape[0] == cap_v
    assert _bytes_equal(captured, eager2)
    assert torch.equal(captured.color[:v], eager2.color) and torch.equal(captured.jacobian[:v], eager2.jacobian)

    flow = models("flow_mlp", 5)
    with pytest.raises(NotImplementedError, match="no Jacobian"):
        flow.extract_mesh(cam, grid, 0.3)
    via_model = flow.extract_mesh(cam, grid, 0.3, want_jacobian=False)
    assert via_model.jacobian is None and via_model.valid()[0] == via_model.vertices.shape[0]


def test_in_frustum_keeps_every_triangle_inside_the_view(models, dev, tmp_path):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import _cameras
    from neural_jacobian_field_amd.field_volume import extract_mesh, mesh_from_values
    model = models("jacobian_mlp", 8)
    grid = _scene_grid((17, 13, 11))
    enc = _encoding(_camera_input(2, dev), 8)
    thr = _median_threshold(_dense_density(model, enc, grid))
    mesh = extract_mesh(model, enc, grid, thr, in_frustum=True)
    everything = extract_mesh(model, enc, grid, thr, in_frustum=False, want_color=False, want_jacobian=False)
    total = 2 * grid.num_nodes
    idx, count = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    hip.field_select(grid.c_grid(), 2, total, idx, count, cams=_cameras(enc, False, action_dim=None))
    inside = np.zeros(total, dtype=bool)
    inside[idx[:int(count.item())].cpu().numpy()] = True
    assert 0.1 * total < inside.sum() < 0.9 * total, "the grid must lie partly outside the view"
    assert 0 < mesh.triangles.shape[0] < everything.triangles.shape[0]
    # the frustum acts as the `valid` mask of the same predicate: no tetrahedron with a corner node outside the view emits
    density = _dense_density(model, enc, grid)
    masked = mesh_from_values(grid, density, thr, valid=torch.from_numpy(inside.reshape(2, -1)).to(dev))
    assert _bytes_equal(mesh, masked)
    _assert_equals_restatement(_numpy(mesh), grid, density.cpu().numpy(), thr, inside.reshape(2, -1))
    nx, ny, nz = grid.dims
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    cell = mesh.triangle_cell.cpu().numpy().astype(np.int64)
    b, local = cell // cells, cell % cells
    ix, iy, iz = local // ((ny - 1) * (nz - 1)), (local // (nz - 1)) % (ny - 1), local % (nz - 1)
    # every vertex of a triangle lies on an edge of its cell whose two end nodes are inside the view
    tri = mesh.triangles.cpu().numpy().astype(np.int64)
    node = mesh.vertex_node.cpu().numpy().astype(np.int64)
    step = np.array(R.DIRECTIONS)[mesh.vertex_edge.cpu().numpy()]
    other = node + step[:, 0] * ny * nz + step[:, 1] * nz + step[:, 2]
    assert inside[node].all() and inside[other].all()
    base = b * grid.num_nodes + (ix * ny + iy) * nz + iz
    for corner in range(3):
        own = node[tri[:, corner]]
        d = own - base                                         # the owner is a corner of the triangle's cell
        assert np.isin(d, [cx * ny * nz + cy * nz + cz for cx in (0, 1) for cy in (0, 1) for cz in (0, 1)]).all()
    # colours and the PLY on a GPU result
    colors = mesh.colors("model_allegro")
    v, t = mesh.valid()
    assert tuple(colors.shape) == (v, 3) and float(colors.min()) >= 0.0 and float(colors.max()) <= 1.0
    assert mesh.save_ply(tmp_path / "mesh.ply", colors=colors) == (v, t)
    raw = open(tmp_path / "mesh.ply", "rb").read()
    payload = raw[raw.index(b"end_header\n") + 11:]
    assert len(payload) == v * 15 + t * 13
    assert np.array_equal(np.frombuffer(payload[:12], dtype="<f4"), mesh.vertices[0].cpu().numpy())
