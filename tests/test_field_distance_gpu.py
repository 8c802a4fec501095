"""GPU tests of the fusion of depth frames into a truncated signed distance and of its sampling (field_volume.fuse_depth /
sample_distance; njf_field_tsdf / njf_field_tsdf_sample) against the numpy restatement of their semantics
(tests/field_distance_restatement.py), in layers, as sections 24 and 26 are, so that exactness is asked only where it can hold.

Layer 1, the projection: a node's pixel and camera z are those ``visible_rows(grid.points(), view)`` reports -- the fusion calls the
device function that ``visible_rows`` calls, and ``visible_rows`` is held to the float64 pinhole model by its own tests.

Layer 2, everything else: from the device's OWN ``pixel`` and ``z`` of the nodes, ``values``, ``weight`` and ``known`` equal the
restatement byte for byte; from the device's own ``values`` and ``weight``, the four outputs of the sampler do.  Outputs are filled
with two different sentinels.

Layer 3 needs no restatement: an identity camera, a constant depth and dyadic coordinates, where every operation is exact.

End to end (the last test): the depth frame of section 22's scene fused on the grid of tests/test_field_distance_cpu.py, the shell
posed at the five commands of section 26 table (c): the planted command has the strictly smallest ``cost()``.  Measured on an
MI355X: 4,238 nodes with a weight, none decided otherwise than by the float64 model; ``cost()`` 5.1221e-3, 1.6289e-2, 1.2732e-2,
8.6199e-3, 1.1129e-2 (restatement 5.1221e-3, 1.6289e-2, 1.2732e-2, 8.6198e-3, 1.1129e-2), margin 3.498e-3.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_distance_restatement as R
import field_visible_restatement as V
from test_field_distance_cpu import E2E_DIMS, E2E_ORIGIN, E2E_STEP, E2E_TRUNCATION, e2e_poses
from test_field_visible_cpu import section_22_scene
from test_field_visible_gpu import _cameras
from test_field_voxels_gpu import HEIGHT, WIDTH

pytestmark = pytest.mark.gpu

F32 = np.float32
ROWS = (1, 63, 64, 65, 257, 4097)
IMAGES = ((1, 1), (1, 7), (5, 3), (48, 64))
PROBLEMS = ((1, 1, 1, 1), (3, 3, 3, 3), (3, 3, 1, 3), (1, 3, 3, 1))                 # (V, M, Mq, Mf)
GRIDS = ((1, 1, 1), (2, 2, 2), (3, 5, 7), (16, 16, 17), (65, 9, 9))                 # 4,352 and 5,265 nodes: past 256 and 1,024
LOWER, UPPER = (-0.6, -0.4, 1.0), (0.6, 0.4, 1.7)                                   # in front of section 22's cameras
TRUNCATION = 0.3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _t(dev, v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _grid(dims):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    if dims == (2, 2, 2):                                                           # one cell, well inside every image
        return FieldGrid.from_bounds((-0.25, -0.125, 1.25), (0.25, 0.125, 1.5), dims)
    return FieldGrid.from_bounds((0.0, 0.0, 1.3) if dims == (1, 1, 1) else LOWER, UPPER, dims)


def _depths(rng, m, views, height, width):
    """[M, V, H, W] fp32: depths around the grid's camera z, a third of the pixels zero, a few NaN and inf."""
    depth = rng.uniform(1.7, 3.0, (m, views, height, width)).astype(F32)
    depth[rng.random(depth.shape) < 1 / 3] = 0.0
    for value in (np.nan, np.inf, -np.inf):
        depth[rng.random(depth.shape) < 0.02] = value
    return depth


def _node_projection(dev, grid, view):
    """(pixel [V, N] int64, z [V, N] fp32): the device's own projection of every node."""
    from neural_jacobian_field_amd.field_volume import visible_rows
    vis = visible_rows(grid.points(device=dev), view)
    return _np(vis.pixel[0]).astype(np.int64), _np(vis.z[0])


def _equal(got, want, fields, what):
    for f in fields:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].dtype, got[f].shape)
        differ = int((got[f].view(np.uint8) != want[f].view(np.uint8)).sum())
        assert differ == 0, (what, f, differ)


def _raw_fuse(dev, grid, depth, view, w2c, m, fill, state=None, **kw):
    """hip.field_tsdf on sentinel-filled outputs of the test's own; a dict of numpy arrays."""
    from neural_jacobian_field_amd import hip
    shapes = dict(values=(m, grid.num_nodes), weight=(m, grid.num_nodes), known=(m,))
    out = {f: torch.empty(shapes[f], dtype=dtype, device=dev) for f, dtype in hip.FIELD_TSDF_OUTPUTS}
    for t in out.values():
        t.view(torch.uint8).fill_(fill)
    hip.field_tsdf(grid.c_grid(), depth, view.intrinsics, w2c, TRUNCATION, out, near=view.near,
                   values_in=None if state is None else state[0], weight_in=None if state is None else state[1], **kw)
    return {f: _np(t) for f, t in out.items()}


def _check_fuse(dev, grid, depth, view, state=None, what="", **kw):
    """Two raw calls on outputs filled with different sentinels, and the public function, against the restatement from the
    device's own node projection.  ``state``: (values, weight) numpy arrays.  Returns the restatement's outputs."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldDistance, fuse_depth
    m = depth.shape[0]
    pixel, z = _node_projection(dev, grid, view)
    far, max_weight = kw.get("far", np.inf), kw.get("max_weight", np.inf)
    want = R.fuse(pixel, z, depth, view.near, far, TRUNCATION, max_weight, *(state or (None, None)))
    d, w2c = _t(dev, depth), hip.inverse(view.cam2world)
    for form, fill in (("first", 0x5a), ("second", 0xa5)):
        got = _raw_fuse(dev, grid, d, view, w2c, m, fill, None if state is None else (_t(dev, state[0]), _t(dev, state[1])), **kw)
        _equal(got, want, R.OUT, (what, form))
    into = None if state is None else FieldDistance(grid, float(F32(TRUNCATION)), _t(dev, state[0]), _t(dev, state[1]),
                                                    torch.zeros(m, dtype=torch.int32, device=dev))
    public = fuse_depth(grid, d if m > 1 else d[0], view, TRUNCATION, into=into, **kw)
    assert into is None or public is into
    _equal({f: _np(getattr(public, f)) for f in R.OUT}, want, R.OUT, (what, "fuse_depth"))
    return want


def _rows(rng, grid, sets, n):
    """[sets, n, 3] fp32: rows in and a little around the grid's box; three are not finite."""
    lower = np.float64(grid.origin)
    upper = lower + np.float64(grid.step) * (np.float64(grid.dims) - 1)
    pad = 0.1 * (upper - lower)
    pts = rng.uniform(lower - pad, upper + pad, (sets, n, 3)).astype(F32)
    nodes = _np(grid.points())[rng.integers(0, grid.num_nodes, (sets, n))]        # a few rows exactly on nodes, the last planes included
    pts = np.where((rng.random((sets, n)) < 0.1)[..., None], nodes, pts)
    if n >= 8:
        pts[:, 3, 1], pts[:, n // 2, 0], pts[:, -2] = np.nan, np.inf, -np.inf
    return pts


def _check_sample(dev, grid, pts, values, weight, m, count=None, labels=None, what=""):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldDistance, sample_distance
    n = pts.shape[1]
    want = R.sample(pts, grid.origin, grid.step, grid.dims, values, weight, count, labels, problems=m)
    p, c, l = _t(dev, pts), (None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)), _t(dev, labels)
    v, w = _t(dev, values), _t(dev, weight)
    shapes = dict(state=(m, n), distance=(m, n), gradient=(m, n, 3), states=(m, hip.FIELD_TSDF_STATES))
    for form, fill in (("first", 0x5a), ("second", 0xa5)):
        out = {f: torch.empty(shapes[f], dtype=dtype, device=dev) for f, dtype in hip.FIELD_TSDF_SAMPLE_OUTPUTS}
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
        hip.field_tsdf_sample(p, grid.c_grid(), v, w, out, m, count=c, labels=l)
        _equal({f: _np(t) for f, t in out.items()}, want, R.SAMPLE_OUT, (what, form))
    if max(pts.shape[0], values.shape[0]) == m:
        field = FieldDistance(grid, TRUNCATION, v, w, torch.zeros(values.shape[0], dtype=torch.int32, device=dev))
        public = sample_distance(p if pts.shape[0] > 1 else p[0], field, labels=l, count=c)
        _equal({f: _np(getattr(public, f)) for f in R.SAMPLE_OUT}, want, R.SAMPLE_OUT, (what, "sample_distance"))
        assert np.allclose(_np(public.cost()), R.cost(want["state"], want["distance"]), rtol=1e-12, atol=0.0, equal_nan=True)
    return want


# ---- 1. the layers over the shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", GRIDS)
def test_every_output_equals_the_restatement(dev, dims):
    from neural_jacobian_field_amd.field_volume import FieldView
    rng = np.random.default_rng(1000 * dims[0] + dims[2])
    grid = _grid(dims)
    case, rows_seen, totals, known, clipped = 0, set(), np.zeros(R.STATES, np.int64), 0, 0
    for height, width in IMAGES:
        for views, m, mq, mf in PROBLEMS:
            n = ROWS[case % len(ROWS)]
            what = f"{dims}, {height} x {width}, n {n}, V {views}, M {m}, Mq {mq}, Mf {mf}"
            case += 1
            k, c2w = _cameras(views)
            view = FieldView(_t(dev, k), _t(dev, c2w), height, width, near=0.0 if case % 2 else 1.9)
            fresh = _check_fuse(dev, grid, _depths(rng, mf, views, height, width), view, what=what + ", fresh")
            kw = dict(far=2.8, max_weight=float(1 + case % 3)) if case % 4 else {}
            field = _check_fuse(dev, grid, _depths(rng, mf, views, height, width), view, (fresh["values"], fresh["weight"]),
                                what=what + ", into", **kw)
            assert (field["weight"] >= fresh["weight"]).all() or "max_weight" in kw
            known += int(field["known"].sum())
            clipped += int((field["values"] == F32(TRUNCATION)).sum())
            if dims == (1, 1, 1):
                continue                                                            # (no cell: the sampler refuses the grid)
            count = None if case % 3 else max(n - 3, 0)
            labels = None if case % 4 or n < 8 else np.where(rng.random(n) < 0.1, -1, rng.integers(0, 3, n)).astype(np.int32)
            got = _check_sample(dev, grid, _rows(rng, grid, mq, n), field["values"], field["weight"], m, count, labels, what)
            assert (got["states"].sum(axis=1) == n).all()
            rows_seen.add(n)
            totals += got["states"].sum(axis=0)
    print(f"{dims}: {case} cases, nodes with a weight {known}, at the truncation {clipped}, states {totals.tolist()}")
    assert known > 0
    if dims != (1, 1, 1):
        assert rows_seen == set(ROWS) and totals.all()
    if grid.num_nodes > 100:
        assert clipped > 0


def test_three_single_view_updates_against_one_call_of_three_views(dev):
    """The same three images through one call and through three: equal ``weight`` bytes; the ``values`` of each route equal that
    route's restatement (the mean is taken in a different order, so they differ from each other in the last bits)."""
    from neural_jacobian_field_amd.field_volume import FieldView
    rng = np.random.default_rng(7)
    grid = _grid((16, 16, 17))
    k, c2w = _cameras(3)
    height, width = 48, 64
    depth = _depths(rng, 3, 3, height, width)
    at_once = _check_fuse(dev, grid, depth, FieldView(_t(dev, k), _t(dev, c2w), height, width), what="three views")
    state = None
    for v in range(3):
        view = FieldView(_t(dev, k[v:v + 1]), _t(dev, c2w[v:v + 1]), height, width)
        step = _check_fuse(dev, grid, depth[:, v:v + 1], view, state, what=f"view {v} alone")
        state = (step["values"], step["weight"])
    assert step["weight"].tobytes() == at_once["weight"].tobytes() and step["known"].tobytes() == at_once["known"].tobytes()
    assert set(np.unique(at_once["weight"]).tolist()) == {0.0, 1.0, 2.0, 3.0}
    both = at_once["weight"] > 0
    print("values that differ between the routes:", int((step["values"][both] != at_once["values"][both]).sum()), "of", int(both.sum()))


# ---- 2. no restatement: an identity camera, a constant depth, dyadic coordinates ------------------------------------------------------------
D0 = 1.09375                                                                       # between the node planes 1.0625 and 1.125


def _exact_scene(dev, z0=0.75, nz=13, **kw):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldView, fuse_depth
    grid = FieldGrid((-0.25, -0.25, z0), (0.125, 0.125, 0.0625), (5, 5, nz))
    k = torch.tensor([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]], device=dev)
    view = FieldView(k, torch.eye(4, device=dev)[None], 8, 8)
    field = fuse_depth(grid, torch.full((1, 8, 8), D0, device=dev), view, 0.25, **kw)
    return grid, view, field


def test_a_constant_depth_through_an_identity_camera_is_exact(dev):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import sample_distance
    grid, view, field = _exact_scene(dev)
    z = grid.points(device=dev)[:, 2]
    s = D0 - z
    seen = s >= -0.25
    assert 0 < int(seen.sum()) < grid.num_nodes and int(field.known[0]) == int(seen.sum())
    assert torch.equal(field.weight[0], seen.to(torch.float32)) and torch.isnan(field.values[0][~seen]).all()
    assert torch.equal(field.values[0][seen], s[seen].clamp(max=0.25)) and int((s > 0.25).sum()) > 0
    # inside the band every corner is unclipped: the interpolant is d0 - z and its derivative (0, 0, -1), exactly
    rng = np.random.default_rng(3)
    pts = torch.from_numpy(np.stack([rng.integers(-256, 257, 500) / 1024, rng.integers(-256, 257, 500) / 1024,
                                     rng.integers(896, 1344, 500) / 1024], axis=1).astype(F32)).to(dev)       # z in [0.875, 1.3125)
    got = sample_distance(pts, field)
    assert (got.state == hip.FIELD_TSDF_KNOWN).all() and got.states.tolist() == [[0, 0, 500]]
    assert torch.equal(got.distance[0], D0 - pts[:, 2])
    assert (got.gradient[0] == torch.tensor([0.0, 0.0, -1.0], device=dev)).all()
    targets, information = got.surface_targets(pts)
    assert torch.equal(targets[0, :, :2], pts[:, :2]) and (targets[0, :, 2] == D0).all() and torch.isfinite(information).all()
    assert float(got.cost()[0]) == float((D0 - pts[:, 2]).double().abs().mean())
    # the fused surface is the plane z = d0
    mesh = field.mesh()
    vertices = mesh.vertices
    assert vertices.shape[0] > 20 and mesh.triangles.shape[0] > 20 and (vertices[:, 2] == D0).all()


def test_rows_behind_the_camera_not_finite_from_the_count_on_and_of_a_negative_label(dev):
    from neural_jacobian_field_amd.field_volume import sample_distance
    grid, view, field = _exact_scene(dev, z0=-0.25, nz=29)                        # node planes from -0.25 (behind the camera) to 1.5
    x, y, z = grid.points(device=dev).unbind(dim=1)
    u, v = x / z + 0.5, y / z + 0.5                                                # the unit pinhole, as the kernel rounds it
    inside = (z > 0) & (u >= 0) & (u < 1) & (v >= 0) & (v < 1)
    assert torch.equal(field.weight[0] > 0, inside & (D0 - z >= -0.25)) and int((z <= 0).sum()) == 125
    assert 0 < int((inside & (z < 0.5)).sum()) < int((z < 0.5).sum())              # near the camera the grid is wider than the image
    pts = F32([[0.0, 0.0, 1.0],            # 0: known
               [0.0, 0.0, -0.125],         # 1: in the grid, behind the camera: no view saw its cell
               [0.0, 0.0, 0.03125],        # 2: a cell with corners on the camera plane z = 0
               [np.nan, 0.0, 1.0],         # 3: not finite
               [0.0, np.inf, 1.0],         # 4: not finite
               [0.0, 0.0, 1.0],            # 5: label -1
               [0.0, 0.0, 1.4],            # 6: further than the truncation behind the surface
               [0.3, 0.0, 1.0],            # 7: outside the grid
               [0.0, 0.0, 1.0],            # 8: from the count on
               [0.0, 0.0, 1.0]])
    labels = torch.tensor([0, 0, 0, 0, 0, -1, 2, 0, 0, 0], dtype=torch.int32, device=dev)
    got = sample_distance(_t(dev, pts), field, labels=labels, count=torch.tensor([8], dtype=torch.int32, device=dev))
    assert got.state.tolist() == [[2, 1, 1, 0, 0, 0, 1, 0, 0, 0]] and got.states.tolist() == [[6, 3, 1]]
    assert got.distance[0, 0] == D0 - 1.0 and torch.isnan(got.distance[0, 1:]).all() and torch.isnan(got.gradient[0, 1:]).all()
    want = R.sample(pts, grid.origin, grid.step, grid.dims, _np(field.values), _np(field.weight), 8, _np(labels))
    for f in R.SAMPLE_OUT:
        assert _np(getattr(got, f)).tobytes() == want[f].tobytes(), f


def test_in_place_and_out_of_place_updates_give_equal_bytes(dev):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldDistance, FieldView, fuse_depth
    rng = np.random.default_rng(13)
    grid = _grid((16, 16, 17))
    k, c2w = _cameras(3)
    view = FieldView(_t(dev, k), _t(dev, c2w), 48, 64)
    first, second = (_t(dev, _depths(rng, 3, 3, 48, 64)) for _ in range(2))
    a = fuse_depth(grid, first, view, TRUNCATION)
    before = {f: getattr(a, f).clone() for f in R.OUT}
    out = {f: torch.empty_like(before[f]) for f in R.OUT}
    hip.field_tsdf(grid.c_grid(), second, view.intrinsics, hip.inverse(view.cam2world), TRUNCATION, out, max_weight=4.0,
                   values_in=a.values, weight_in=a.weight)
    for f in R.OUT:
        assert torch.equal(_bytes(getattr(a, f)), _bytes(before[f])), f              # the state was read only
    b = fuse_depth(grid, second, view, TRUNCATION, max_weight=4.0, into=a)
    assert b is a and isinstance(b, FieldDistance)
    for f in R.OUT:
        assert torch.equal(_bytes(getattr(b, f)), _bytes(out[f])), f
    assert not torch.equal(_bytes(b.values), _bytes(before["values"])) and float(b.weight.max()) == 4.0


# ---- 3. determinism -------------------------------------------------------------------------------------------------------------------------
def test_seven_calls_and_two_replays_of_a_capture_give_equal_bytes(dev):
    from neural_jacobian_field_amd.field_volume import FieldView, fuse_depth, sample_distance
    rng = np.random.default_rng(11)
    grid = _grid((65, 9, 9))
    k, c2w = _cameras(2)
    view = FieldView(_t(dev, k), _t(dev, c2w), 12, 16)
    depth = _t(dev, _depths(rng, 2, 2, 12, 16))
    pts = _t(dev, _rows(rng, grid, 2, 4097))

    def run():
        field = fuse_depth(grid, depth, view, TRUNCATION, max_weight=1.5)
        return field, sample_distance(pts, field)

    first = run()
    assert int(first[0].known.min()) > 100 and (first[1].states.sum(dim=1) == 4097).all() and int(first[1].states[:, 2].min()) > 0
    pairs = lambda result: [(f, getattr(result[0], f)) for f in R.OUT] + [(f, getattr(result[1], f)) for f in R.SAMPLE_OUT]   # noqa: E731
    for _ in range(6):
        for (f, a), (_, b) in zip(pairs(run()), pairs(first)):
            assert torch.equal(_bytes(a), _bytes(b)), f
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _, t in pairs(out):
        t.view(torch.uint8).fill_(0x77)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for (f, a), (_, b) in zip(pairs(out), pairs(first)):
        assert torch.equal(_bytes(a), _bytes(b)), f


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------------
def test_the_planted_command_has_the_smallest_cost_in_the_fused_frame(dev):
    """Section 22's depth frame fused on the grid of tests/test_field_distance_cpu.py; the shell posed at the five commands of
    section 26 table (c).  The restatement alone meets the condition (5.12e-3 against 8.62e-3 for the runner-up: the CPU test)."""
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldView, fuse_depth, sample_distance
    s, k, c2w, planted, depth, _ = section_22_scene()
    poses = e2e_poses(s, planted)
    grid = FieldGrid(E2E_ORIGIN, E2E_STEP, E2E_DIMS)
    view = FieldView(_t(dev, k), _t(dev, c2w), HEIGHT, WIDTH)
    field = fuse_depth(grid, _t(dev, depth.astype(F32)), view, E2E_TRUNCATION)
    got = sample_distance(_t(dev, poses), field)
    cost = _np(got.cost())
    want_field = R.fuse_depth(E2E_ORIGIN, E2E_STEP, E2E_DIMS, depth[None], k, c2w, 0.0, np.inf, E2E_TRUNCATION)
    want = R.sample(poses, E2E_ORIGIN, E2E_STEP, E2E_DIMS, want_field["values"], want_field["weight"])
    print("known nodes", field.known.tolist(), "(restatement", want_field["known"].tolist(), ") states", got.states.tolist(), "cost",
          [f"{c:.4e}" for c in cost], "(restatement", [f"{c:.4e}" for c in R.cost(want["state"], want["distance"])],
          f") margin {cost[1:].min() - cost[0]:.3e}; nodes whose weight differs from the float64 model's:",
          int((_np(field.weight) != want_field["weight"]).sum()))
    assert (got.states.sum(dim=1) == 878).all() and int(got.states[:, 0].max()) == 0
    assert all(cost[0] < c for c in cost[1:])
