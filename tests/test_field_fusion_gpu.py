"""GPU tests of the multi-view fusion (field_volume.fuse_views, extract_field / extract_mesh with ``views_per_scene``;
njf_field_fuse / njf_field_combine).

``fuse_views`` is compared bit for bit with the numpy restatement of the semantics (tests/field_fusion_restatement.py), the
reference ``s_v`` being the existing per-view frustum selection (``hip.field_select``).  The fused extractions are compared
with that route on the dense per-view densities (indices, density, coordinates, view masks, mesh geometry: bit for bit) and
with the float64 combination of the device's own per-view rows (colour, Jacobian) under the bound
``2 * (2V + 2) * 2**-24 * max_v |x_v|`` per element: the first-order rounding bound of the V-term fma chain, the weight sum
and one division, doubled for the higher-order terms.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_fusion_restatement as R
import field_mesh_restatement as MR

pytestmark = pytest.mark.gpu

IMG = 64
# (dims, scenes, views): 9x8x7 and 17x13x11 are no multiple of the 1024-node workgroup (a ragged tail, for 2431 nodes after
# two full ones); 40^3 spans 63 workgroups
SMALL = [((9, 8, 7), 2, 2), ((17, 13, 11), 1, 3)]
LARGE = ((40, 40, 40), 1, 2)
# camera centres of the views of a scene: together with the identity view they see the scene grid partly, so that nodes
# seen by no view, by some and by all of them exist
OFFSETS = ((0.0, 0.0, 0.0), (0.62, 0.05, 0.0), (-0.5, -0.06, 0.1))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


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


def _poses(scenes, views):
    """[G*V, 4, 4] camera-to-world: view v of scene g looks from OFFSETS[v] (moved a little per scene) with a small rotation."""
    from neural_jacobian_field_amd import synthetic
    c2w = synthetic.general_pose(7, scenes * views, scale=0.04)
    for g in range(scenes):
        for v in range(views):
            c2w[g * views + v, :3, 3] = torch.tensor(OFFSETS[v]) + 0.03 * g
    c2w[0] = torch.eye(4)
    return c2w


def _encoding(scenes, views, dev, adim=8, seed=1, c2w=None):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    b = scenes * views
    c2w = _poses(scenes, views) if c2w is None else c2w
    k = synthetic.synthetic_cameras(b)["ctxt_k_norm"]
    return PixelEncoding(features=synthetic.synthetic_features(b, IMG, IMG, seed=seed).to(dev), extrinsics=c2w.to(dev),
                         intrinsics=k.to(dev), action=synthetic.synthetic_action(b, adim).to(dev))


def _view(enc, rows):
    """The PixelEncoding of some batch elements of ``enc``."""
    from neural_jacobian_field_amd.decoder import PixelEncoding
    rows = list(rows)
    return PixelEncoding(features=enc.features[rows].contiguous(), extrinsics=enc.extrinsics[rows].contiguous(),
                         intrinsics=enc.intrinsics[rows].contiguous(), action=enc.action[rows].contiguous())


def _seen_per_view(grid, enc):
    """[B, N] bool from the existing frustum selection (the definition of s_v)."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import _cameras
    b = enc.extrinsics.shape[0]
    total = b * grid.num_nodes
    dev = enc.extrinsics.device
    idx, count = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    hip.field_select(grid.c_grid(), b, total, idx, count, cams=_cameras(enc, False, action_dim=None))
    inside = np.zeros(total, dtype=bool)
    inside[idx[:int(count.item())].cpu().numpy()] = True
    return inside.reshape(b, grid.num_nodes)


def _frustum_margin(enc, xyz, scene, views):
    """[n, V] float64: how far inside (> 0) or outside (< 0) the frustum of each view of its scene a position lies."""
    w2c = np.linalg.inv(enc.extrinsics.double().cpu().numpy())
    k = enc.intrinsics.double().cpu().numpy()
    x = xyz.double().cpu().numpy()
    out = np.empty((x.shape[0], views))
    for v in range(views):
        b = scene.cpu().numpy().astype(np.int64) * views + v
        cam = np.einsum("nij,nj->ni", w2c[b, :3, :3], x) + w2c[b, :3, 3]
        uvw = np.einsum("nij,nj->ni", k[b], cam)
        u, w = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
        out[:, v] = np.minimum.reduce([cam[:, 2], u, 1 - u, w, 1 - w])
    return out


def _analytic(grid, batch):
    """[B, N] fp32 > 0: a different smooth field per batch element, with exact ties between views sprinkled in."""
    pts = MR.grid_points(grid.origin, grid.step, grid.dims)
    rows = np.stack([np.exp(MR.smooth_random_field(pts, seed=21 + b)).astype(np.float32) for b in range(batch)])
    rows[:, ::17] = rows[0, ::17]
    return rows


def _dense_density(model, enc, grid):
    """The existing dense route: grid.points() + compute_density -> [B, N]."""
    b = enc.extrinsics.shape[0]
    xyz = grid.points(device=enc.extrinsics.device)
    head, _ = model.compute_density(xyz[None].expand(b, -1, 3).contiguous(), enc)
    return head.density.reshape(b, grid.num_nodes).clone()


def _median_of_valid(fused, valid):
    """Half-way between the two middle fused values of the valid nodes: no node sits on the threshold."""
    s = torch.sort(fused[valid].double().cpu()).values
    k = s.numel() // 2
    return float(0.5 * (s[k - 1] + s[k]))


def _per_view_rows(model, enc, grid, views, node, xyz=None):
    """The device's own per-view outputs at the entries ``node`` (fused global indices; at the positions ``xyz`` if given):
    (density [n, V], color [n, V, 3], jacobian [n, V, 3A]) as numpy."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import _cameras, _map_of
    dec = model.decoder
    dev = node.device
    nodes, n, a_dim = grid.num_nodes, node.numel(), dec.kernel_action_dim
    g, local = node.long() // nodes, node.long() % nodes
    expanded = (((g * views)[:, None] + torch.arange(views, device=dev)[None]) * nodes + local[:, None]).reshape(-1).to(torch.int32)
    cams = _cameras(enc, False, action_dim=a_dim)
    w, bd, bc, bj = dec.packed()
    gmap, base = _map_of(dec, enc.features)
    out = (torch.empty(n * views, device=dev), torch.empty(n * views, 3, device=dev), torch.empty(n * views, 3 * a_dim, device=dev))
    kw = dict(goff_density=base + dec.GOFF_DENSITY, goff_jacobian=base + dec.GOFF_JACOBIAN, w_all=w, b_density=bd, b_color=bc,
              b_jacobian=bj, jacobian_kind=dec.JACOBIAN_KIND, density=out[0], color=out[1], jacobian=out[2], precision=dec.precision,
              jacobian_precision=dec.j_precision)
    if xyz is None:
        hip.field_forward(grid.c_grid(), expanded, None, n * views, cams, hip.make_feature_map(gmap), mode=1, **kw)
    else:
        at = xyz[:, None, :].expand(n, views, 3).reshape(-1, 3).contiguous()
        hip.field_forward_at(at, expanded, None, n * views, nodes, cams, hip.make_feature_map(gmap), **kw)
    return (out[0].reshape(n, views).cpu().numpy(), out[1].reshape(n, views, 3).cpu().numpy(),
            out[2].reshape(n, views, 3 * a_dim).cpu().numpy())


def _assert_combination(name, got, density, seen, rows):
    ref, bound = R.combine(density, seen, rows), R.combine_bound(rows)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: max |err| = {float(err.max()) if err.size else 0.0:.3e}, largest err / bound = {worst:.3f}")
    assert (err <= bound).all(), (name, worst)


def _jacobian_rows(jacobian):
    """[n, A, 3] as the kernels' [n, 3A] rows."""
    return jacobian.reshape(jacobian.shape[0], -1).cpu().numpy()


def _with_precision(model, precision):
    from neural_jacobian_field_amd import hip
    model.set_precision(hip.DEFAULT_PRECISION if precision is None else precision)


# ---- 1. fuse_views against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,scenes,views", SMALL + [LARGE])
def test_fuse_views_equals_the_restatement_bit_for_bit(dev, dims, scenes, views):
    from neural_jacobian_field_amd.field_volume import fuse_views
    grid = _scene_grid(dims)
    enc = _encoding(scenes, views, dev)
    values = _analytic(grid, scenes * views)
    dvalues = torch.from_numpy(values).to(dev)
    inside = _seen_per_view(grid, enc)
    count = inside.reshape(scenes, views, -1).sum(axis=1)
    assert (count == 0).any() and ((count > 0) & (count < views)).any() and (count == views).any(), np.bincount(count.ravel())
    for cameras, seen in ((enc, inside), (None, np.ones_like(inside))):
        for mode in R.MODES:
            for min_views in (1, views):
                fused, mask, valid = fuse_views(grid, dvalues, cameras, views_per_scene=views, mode=mode, min_views=min_views)
                assert fused.dtype == torch.float32 and mask.dtype == torch.uint8 and valid.dtype == torch.bool
                assert tuple(fused.shape) == tuple(mask.shape) == tuple(valid.shape) == (scenes, grid.num_nodes)
                ref = R.fuse(values.reshape(scenes, views, -1), seen.reshape(scenes, views, -1), mode, min_views)
                key = (cameras is not None, mode, min_views)
                assert np.array_equal(mask.cpu().numpy(), ref[1]), key
                assert np.array_equal(valid.cpu().numpy(), ref[2]), key
                assert np.array_equal(fused.cpu().numpy().view(np.uint32), ref[0].view(np.uint32)), key


# ---- 2. fused extract_field against the definition ---------------------------------------------------------------------------------
FIELD_CASES = [(d, g, v, kind, adim, prec) for d, g, v in SMALL
               for kind, adim in (("jacobian_mlp", 8), ("jacobian_transformer", 6)) for prec in ("f32", None)]
FIELD_CASES.append(LARGE + ("jacobian_mlp", 8, None))


@pytest.mark.parametrize("dims,scenes,views,kind,adim,precision", FIELD_CASES)
@pytest.mark.parametrize("mode", ["mean"])
def test_fused_extract_field_equals_the_definition(models, dev, dims, scenes, views, kind, adim, precision, mode):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import extract_field, fuse_views
    model = models(kind, adim)
    _with_precision(model, precision)
    try:
        grid = _scene_grid(dims)
        enc = _encoding(scenes, views, dev, adim)
        fused, mask, valid = fuse_views(grid, _dense_density(model, enc, grid), enc, views_per_scene=views, mode=mode)
        thr = _median_of_valid(fused, valid)
        expect = torch.nonzero((valid & (fused >= thr)).reshape(-1)).reshape(-1)
        assert 0.05 * int(valid.sum()) < expect.numel() < 0.95 * int(valid.sum())
        cloud = extract_field(model, enc, grid, thr, views_per_scene=views, fuse=mode)
        n = cloud.valid()
        assert n == cloud.index.shape[0] == expect.numel() and cloud.index.dtype == torch.int32
        assert torch.equal(cloud.index.long(), expect)
        assert torch.equal(cloud.density, fused.reshape(-1)[expect])
        assert torch.equal(cloud.xyz, grid.points(cloud.index))
        assert cloud.views.dtype == torch.uint8 and torch.equal(cloud.views, mask.reshape(-1)[expect])
        assert torch.equal(cloud.batch_index.long(), expect // grid.num_nodes) and cloud.stage_names == ("density",)
        assert tuple(cloud.color.shape) == (n, 3) and tuple(cloud.jacobian.shape) == (n, adim, 3)
        density, color, jacobian = _per_view_rows(model, enc, grid, views, cloud.index)
        seen = ((cloud.views.cpu().numpy()[:, None] >> np.arange(views)[None]) & 1).astype(bool)
        assert seen.any(axis=1).all() and not seen.all()
        _assert_combination("color", cloud.color.cpu().numpy(), density, seen, color)
        _assert_combination("jacobian", _jacobian_rows(cloud.jacobian), density, seen, jacobian)
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


def test_fused_extract_field_modes_min_views_and_options(models, dev):
    """"min" / "max" with min_views = V, no frustum, colour only / Jacobian only / neither, a threshold <= 0."""
    from neural_jacobian_field_amd.field_volume import extract_field, fuse_views
    model = models("jacobian_mlp", 8)
    (dims, scenes, views) = SMALL[1]
    grid = _scene_grid(dims)
    enc = _encoding(scenes, views, dev)
    dense = _dense_density(model, enc, grid)
    for mode, min_views, frustum in (("min", views, True), ("max", 2, True), ("min", 1, False)):
        fused, mask, valid = fuse_views(grid, dense, enc if frustum else None, views_per_scene=views, mode=mode, min_views=min_views)
        thr = _median_of_valid(fused, valid)
        expect = torch.nonzero((valid & (fused >= thr)).reshape(-1)).reshape(-1)
        cloud = extract_field(model, enc, grid, thr, views_per_scene=views, fuse=mode, min_views=min_views, in_frustum=frustum)
        assert expect.numel() > 0 and torch.equal(cloud.index.long(), expect)
        assert torch.equal(cloud.density, fused.reshape(-1)[expect]) and torch.equal(cloud.views, mask.reshape(-1)[expect])
        if not frustum:
            assert bool((cloud.views == (1 << views) - 1).all())
    # an invalid node (fused = 0) does not pass a threshold <= 0
    fused, mask, valid = fuse_views(grid, dense, enc, views_per_scene=views, min_views=views)
    everything = extract_field(model, enc, grid, -1.0, views_per_scene=views, min_views=views, want_color=False, want_jacobian=False)
    assert 0 < int(valid.sum()) < valid.numel()
    assert torch.equal(everything.index.long(), torch.nonzero(valid.reshape(-1)).reshape(-1))
    assert everything.color is None and everything.jacobian is None
    assert torch.equal(everything.views, mask.reshape(-1)[everything.index.long()])
    # colour only (with a view direction) and Jacobian only share the rows of the full extraction
    thr = _median_of_valid(fused, valid)
    full = extract_field(model, enc, grid, thr, views_per_scene=views, min_views=views)
    no_color = extract_field(model, enc, grid, thr, views_per_scene=views, min_views=views, want_color=False)
    bare = extract_field(model, enc, grid, thr, views_per_scene=views, min_views=views, want_jacobian=False,
                         view_direction=(0.6, -0.48, 0.64))
    assert no_color.color is None and torch.equal(no_color.jacobian, full.jacobian) and torch.equal(no_color.index, full.index)
    assert bare.jacobian is None and torch.equal(bare.index, full.index) and not torch.equal(bare.color, full.color)
    with pytest.raises(ValueError, match="cull"):
        extract_field(model, enc, grid, thr, views_per_scene=views, cull=0.1)


# ---- 3. fused extract_mesh ------------------------------------------------------------------------------------------------------
MESH_FIELDS = ("vertex_node", "vertex_edge", "triangles", "triangle_cell", "vertex_t", "vertices")


def _geometry_equal(a, b):
    return (int(a.vertex_count.item()), int(a.triangle_count.item())) == (int(b.vertex_count.item()), int(b.triangle_count.item())) \
        and all(torch.equal(getattr(a, k), getattr(b, k)) for k in MESH_FIELDS)


@pytest.mark.parametrize("dims,scenes,views,kind,adim,precision", FIELD_CASES[:-1])
def test_fused_extract_mesh_equals_the_definition(models, dev, dims, scenes, views, kind, adim, precision):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import _cameras
    from neural_jacobian_field_amd.field_volume import extract_mesh, fuse_views, mesh_from_values
    model = models(kind, adim)
    _with_precision(model, precision)
    try:
        grid = _scene_grid(dims)
        enc = _encoding(scenes, views, dev, adim)
        fused, mask, valid = fuse_views(grid, _dense_density(model, enc, grid), enc, views_per_scene=views)
        thr = _median_of_valid(fused, valid)
        mesh = extract_mesh(model, enc, grid, thr, views_per_scene=views)
        v, t = mesh.valid()
        assert v == mesh.vertices.shape[0] > 0 and t == mesh.triangles.shape[0] > 0
        assert _geometry_equal(mesh, mesh_from_values(grid, fused, thr, valid=valid)), "geometry differs from the fused values'"
        assert int(mesh.batch_index.max()) == scenes - 1 and tuple(mesh.jacobian.shape) == (v, adim, 3)
        # s_v at the vertex positions: the combine launch alone gives the same bytes, and a float64 projection agrees with
        # them wherever the position is not within 1e-4 of the frustum's boundary
        views_only = torch.empty(v, dtype=torch.uint8, device=dev)
        hip.field_combine(mesh.vertices, mesh.vertex_node, None, v, grid.num_nodes, views, _cameras(enc, False, action_dim=None),
                          None, out_views=views_only)
        assert mesh.vertex_views.dtype == torch.uint8 and torch.equal(mesh.vertex_views, views_only)
        seen = ((mesh.vertex_views.cpu().numpy()[:, None] >> np.arange(views)[None]) & 1).astype(bool)
        margin = _frustum_margin(enc, mesh.vertices, mesh.batch_index, views)
        clear = np.abs(margin) > 1e-4
        assert clear.mean() > 0.9 and np.array_equal(seen[clear], margin[clear] > 0)
        assert seen.all(axis=1).any() and not seen.all(), "vertices seen by every view and by some only must both occur"
        density, color, jacobian = _per_view_rows(model, enc, grid, views, mesh.vertex_node, xyz=mesh.vertices)
        _assert_combination("color", mesh.color.cpu().numpy(), density, seen, color)
        _assert_combination("jacobian", _jacobian_rows(mesh.jacobian), density, seen, jacobian)
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


# ---- 4. duplicate views ----------------------------------------------------------------------------------------------------------
def test_two_copies_of_one_view_fuse_to_that_view(models, dev):
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models("jacobian_mlp", 8)
    grid = _scene_grid((17, 13, 11))
    one = _view(_encoding(1, 2, dev), [1])
    twice = _view(one, [0, 0])
    single = None
    for mode in R.MODES:
        if single is None:
            dense = _dense_density(model, one, grid)
            thr = float(torch.quantile(dense.double().cpu(), 0.5))
            single = extract_field(model, one, grid, thr)
            assert 0 < single.index.shape[0] < grid.num_nodes
        cloud = extract_field(model, twice, grid, thr, views_per_scene=2, fuse=mode)
        assert torch.equal(cloud.index, single.index), mode                   # (d + d) / 2 is exact
        assert torch.equal(cloud.density, single.density) and torch.equal(cloud.xyz, single.xyz), mode
        assert bool((cloud.views == 3).all())
        rows = lambda t: np.stack([t.cpu().numpy()] * 2, axis=1)             # noqa: E731
        density = rows(single.density)
        seen = np.ones_like(density, dtype=bool)
        _assert_combination("color", cloud.color.cpu().numpy(), density, seen, rows(single.color))
        _assert_combination("jacobian", _jacobian_rows(cloud.jacobian), density, seen, rows(single.jacobian.reshape(-1, 24)))


# ---- 5. carving --------------------------------------------------------------------------------------------------------------------
def test_min_carves_what_one_view_alone_would_keep(models, dev):
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models("jacobian_mlp", 8)
    grid = _scene_grid((17, 13, 11))
    enc = _encoding(1, 2, dev)
    thr = float(torch.quantile(_dense_density(model, enc, grid).double().cpu(), 0.5))
    carved = set(extract_field(model, enc, grid, thr, views_per_scene=2, fuse="min", min_views=2).index.cpu().tolist())
    alone = [set(extract_field(model, _view(enc, [v]), grid, thr).index.cpu().tolist()) for v in (0, 1)]
    assert carved and carved <= alone[0] and carved <= alone[1]
    assert (alone[0] - alone[1]) and (alone[1] - alone[0]), "each view must keep nodes the other one rejects"
    assert not (alone[0] ^ alone[1]) & carved


# ---- 6. forms ----------------------------------------------------------------------------------------------------------------------
CLOUD_FIELDS = ("index", "xyz", "density", "color", "jacobian", "views")
FUSED_MESH_FIELDS = MESH_FIELDS + ("color", "jacobian", "vertex_views")


def _rows_equal(a, b, fields, rows):
    return all(torch.equal(getattr(a, k)[:(rows[1] if k.startswith("tri") else rows[0])],
                           getattr(b, k)[:(rows[1] if k.startswith("tri") else rows[0])]) for k in fields)


def test_cloud_forms_eager_capacity_truncation_and_capture(models, dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models("jacobian_mlp", 8)
    dims, scenes, views = SMALL[0]
    grid = _scene_grid(dims)
    enc = _encoding(scenes, views, dev)
    thr = float(torch.quantile(_dense_density(model, enc, grid).double().cpu(), 0.5))
    kw = dict(views_per_scene=views, fuse="mean")
    eager = extract_field(model, enc, grid, thr, **kw)
    n = eager.valid()
    assert n == eager.index.shape[0] > 40 and _rows_equal(eager, extract_field(model, enc, grid, thr, **kw), CLOUD_FIELDS, (n, 0))
    padded = extract_field(model, enc, grid, thr, max_points=n + 29, **kw)
    assert padded.index.shape[0] == n + 29 and padded.valid() == n and _rows_equal(padded, eager, CLOUD_FIELDS, (n, 0))
    short = extract_field(model, enc, grid, thr, max_points=n - 17, **kw)
    assert int(short.count.item()) == n and short.valid() == n - 17 and _rows_equal(short, eager, CLOUD_FIELDS, (n - 17, 0))
    enc2 = PixelEncoding(features=synthetic.synthetic_features(scenes * views, IMG, IMG, seed=9).to(dev), extrinsics=enc.extrinsics,
                         intrinsics=enc.intrinsics, action=None)
    eager2 = extract_field(model, enc2, grid, thr, **kw)
    cap = max(n, eager2.valid()) + 31
    static = PixelEncoding(features=enc.features.clone(), extrinsics=enc.extrinsics, intrinsics=enc.intrinsics, action=None)
    extract_field(model, static, grid, thr, max_points=cap, **kw)                # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = extract_field(model, static, grid, thr, max_points=cap, **kw)
    static.features.copy_(enc2.features)
    graph.replay()
    torch.cuda.synchronize()
    assert captured.valid() == eager2.valid() != n
    assert _rows_equal(captured, eager2, CLOUD_FIELDS, (eager2.valid(), 0))


def test_mesh_forms_eager_capacity_truncation_and_capture(models, dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import extract_mesh
    model = models("jacobian_mlp", 8)
    dims, scenes, views = SMALL[0]
    grid = _scene_grid(dims)
    enc = _encoding(scenes, views, dev)
    thr = float(torch.quantile(_dense_density(model, enc, grid).double().cpu(), 0.5))
    kw = dict(views_per_scene=views, fuse="mean")
    eager = extract_mesh(model, enc, grid, thr, **kw)
    v, t = eager.valid()
    assert v > 40 and t > 40 and _rows_equal(eager, extract_mesh(model, enc, grid, thr, **kw), FUSED_MESH_FIELDS, (v, t))
    padded = extract_mesh(model, enc, grid, thr, max_vertices=v + 13, max_triangles=t + 7, **kw)
    assert padded.vertices.shape[0] == v + 13 and padded.valid() == (v, t) and _rows_equal(padded, eager, FUSED_MESH_FIELDS, (v, t))
    short = extract_mesh(model, enc, grid, thr, max_vertices=v - 11, max_triangles=t // 2, **kw)
    assert (int(short.vertex_count.item()), int(short.triangle_count.item())) == (v, t)
    assert short.valid() == (v - 11, t // 2) and _rows_equal(short, eager, FUSED_MESH_FIELDS, (v - 11, t // 2))
    enc2 = PixelEncoding(features=synthetic.synthetic_features(scenes * views, IMG, IMG, seed=9).to(dev), extrinsics=enc.extrinsics,
                         intrinsics=enc.intrinsics, action=None)
    eager2 = extract_mesh(model, enc2, grid, thr, **kw)
    v2, t2 = eager2.valid()
    caps = dict(max_vertices=max(v, v2) + 50, max_triangles=max(t, t2) + 50)
    static = PixelEncoding(features=enc.features.clone(), extrinsics=enc.extrinsics, intrinsics=enc.intrinsics, action=None)
    extract_mesh(model, static, grid, thr, **caps, **kw)                         # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = extract_mesh(model, static, grid, thr, **caps, **kw)
    static.features.copy_(enc2.features)
    graph.replay()
    torch.cuda.synchronize()
    assert captured.valid() == (v2, t2) != (v, t)
    assert _rows_equal(captured, eager2, FUSED_MESH_FIELDS, (v2, t2))


# ---- 7. a single view per scene is today's code path ---------------------------------------------------------------------------------
def test_views_per_scene_one_changes_nothing(models, dev):
    from neural_jacobian_field_amd.field_volume import extract_field, extract_mesh
    model = models("jacobian_mlp", 8)
    grid = _scene_grid((9, 8, 7))
    enc = _encoding(2, 2, dev)
    thr = float(torch.quantile(_dense_density(model, enc, grid).double().cpu(), 0.5))
    plain, keyed = extract_field(model, enc, grid, thr), extract_field(model, enc, grid, thr, views_per_scene=1)
    assert plain.views is None and keyed.views is None and plain.stage_names == keyed.stage_names
    assert plain.index.shape[0] > 0 and _rows_equal(plain, keyed, CLOUD_FIELDS[:-1], (plain.index.shape[0], 0))
    culled = extract_field(model, enc, grid, thr, cull=0.0, views_per_scene=1)
    assert culled.stage_names == ("frustum", "proposal", "density")
    plain, keyed = extract_mesh(model, enc, grid, thr), extract_mesh(model, enc, grid, thr, views_per_scene=1)
    assert plain.vertex_views is None and keyed.vertex_views is None
    assert plain.valid()[1] > 0 and _rows_equal(plain, keyed, FUSED_MESH_FIELDS[:-1], plain.valid())
