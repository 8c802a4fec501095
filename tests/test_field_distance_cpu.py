"""Host-side tests of the fusion of depth frames into a truncated signed distance and of its sampling (field_volume.fuse_depth /
sample_distance; njf_field_tsdf / njf_field_tsdf_sample): the numpy restatement
(tests/field_distance_restatement.py) against cases written out by hand -- the truncation rule at equality on both sides, ``near < d
<= far`` at both ends, depths that are not numbers, the three update cases, a row on the last node plane and one an ulp outside
the grid, one corner without a weight --, ``cost()`` and ``surface_targets`` on the CPU, the signatures, every argument check,
raised before any device work (there is no GPU here), the C ABI's symbols and return codes, and the condition the GPU's end-to-end
test relies on: the restated ``cost()`` of the section-22 shell at the five commands of section 26 table (c).

Measured here, grid [-0.75, 0.75] x [-0.625, 0.625] x [0.875, 1.875] at step 1/32 (49 x 41 x 33 nodes), truncation 1/16: ``cost()``
5.12e-3 at the planted command, 1.629e-2, 1.273e-2, 8.62e-3 and 1.113e-2 at the four others: the margin is 3.50e-3."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_commands_restatement as F
import field_distance_restatement as R
from test_field_frame_cpu import COMMANDS
from test_field_visible_cpu import _bad_views, _view, section_22_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
DEFAULT = object()

# the end-to-end grid (shared with the GPU test): dyadic bounds around every pose of the shell, step 1/32, truncation two steps
E2E_ORIGIN, E2E_STEP, E2E_DIMS, E2E_TRUNCATION = (-0.75, -0.625, 0.875), (0.03125,) * 3, (49, 41, 33), 0.0625
E2E_COST = (5.12e-3, 1.629e-2, 1.273e-2, 8.62e-3, 1.113e-2)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


def up(x):
    return np.nextafter(F32(x), INF)


def down(x):
    return np.nextafter(F32(x), -INF)


def _one_view(depths, z, **kw):
    """``fuse`` of one view of 1 x n pixels: node i has pixel i, depth ``depths[i]`` and camera z ``z[i]``."""
    depths, z = F32(depths), F32(z)
    n = depths.size
    args = dict(near=0.0, far=np.inf, truncation=0.25)
    args.update(kw)
    return R.fuse(np.arange(n)[None], z[None], depths.reshape(1, 1, 1, n), **args)


def _same(a, b):
    return np.asarray(a, F32).tobytes() == np.asarray(b, F32).tobytes()


# ---- the rule of the fusion -----------------------------------------------------------------------------------------------------------------
def test_the_truncation_rule_at_equality_on_both_sides():
    # z = 1, truncation 1/4: every difference below is exact in fp32
    got = _one_view([0.75, down(0.75), 1.25, up(1.25), 1.0, 3.0], [1.0] * 6)
    assert _same(got["values"], [[-0.25, NAN, 0.25, 0.25, 0.0, 0.25]])      # s == -t contributes; s == t is t itself; above: clipped
    assert _same(got["weight"], [[1, 0, 1, 1, 1, 1]]) and got["known"].tolist() == [5]
    # a truncation that is not exact: the rule is the fp32 subtraction against the fp32 truncation, whatever they round to
    t, z = F32(0.1), F32(1.3)
    for d in (F32(z - t), down(z - t), up(z - t), F32(z + t), up(z + t)):
        s = F32(d - z)
        want = NAN if not s >= -t else min(s, t)
        assert _same(_one_view([d], [z], truncation=0.1)["values"], [[want]]), d


def test_near_and_far_at_both_ends_and_depths_that_are_no_numbers():
    got = _one_view([0.5, up(0.5), 2.0, up(2.0), 1.0], [0.5, 0.5, 2.0, 2.0, 1.0], near=0.5, far=2.0)
    assert _same(got["weight"], [[0, 1, 1, 0, 1]])                          # near < d <= far
    assert _same(got["values"], [[NAN, 2.0 ** -24, 0.0, NAN, 0.0]])
    got = _one_view([np.nan, np.inf, -np.inf, 0.0, -1.0, 1.0], [1.0] * 6)
    assert _same(got["weight"], [[0, 0, 0, 0, 0, 1]]) and got["known"].tolist() == [1]
    assert _same(got["values"], [[NAN] * 5 + [0.0]])
    # a node with no pixel, and a node whose camera z is NaN: no view contributes
    got = R.fuse(np.int64([[-1, 0]]), F32([[1.0, np.nan]]), np.ones((1, 1, 1, 1), F32), 0.0, np.inf, 0.25)
    assert _same(got["weight"], [[0, 0]]) and _same(got["values"], [[NAN, NAN]])


def test_the_three_update_cases_and_the_clamp():
    # three views of one pixel each, four nodes at z = 1; node 3 has no pixel in any view
    pixel = np.int64([[0, 0, 0, -1]] * 3)
    z = np.ones((3, 4), F32)
    depth = F32([2.0, 0.875, 0.0]).reshape(1, 3, 1, 1)                      # s = 0.25 (clipped from 1), -0.125, no return
    fresh = R.fuse(pixel, z, depth, 0.0, np.inf, 0.25)
    assert _same(fresh["values"], [[0.0625] * 3 + [NAN]]) and _same(fresh["weight"], [[2, 2, 2, 0]]) and fresh["known"].tolist() == [3]
    assert _same(R.fuse(pixel, z, depth, 0.0, np.inf, 0.25, max_weight=1.5)["weight"], [[1.5, 1.5, 1.5, 0]])
    # a state: W0 == 0 with a NaN value (not read), W0 > 0, and the node no view sees (copied through)
    v0, w0 = F32([[NAN, 0.5, 7.0, -3.0]]), F32([[0, 2, 0, 5]])
    got = R.fuse(pixel, z, depth, 0.0, np.inf, 0.25, max_weight=3.0, values_in=v0, weight_in=w0)
    assert _same(got["values"], [[0.0625, (2 * 0.5 + 0.125) / 4, 0.0625, -3.0]])
    assert _same(got["weight"], [[2, 3, 2, 5]]) and got["known"].tolist() == [4]     # min(2 + 2, 3); the copied weight is not clamped
    none = R.fuse(pixel, z, np.zeros((1, 3, 1, 1), F32), 0.0, np.inf, 0.25, values_in=v0, weight_in=w0)
    assert _same(none["values"], v0) and _same(none["weight"], w0) and none["known"].tolist() == [2]
    # the sum is taken in ascending view order, in fp32: (1 + 2^-24) + 2^-24 is 1, 1 + (2^-24 + 2^-24) is not
    quarter = np.full((3, 4), 0.25, F32)
    depth = F32([2.0, 0.25 + 2.0 ** -24, 0.25 + 2.0 ** -24]).reshape(1, 3, 1, 1)          # s = 1 (clipped), 2^-24, 2^-24
    assert _same(R.fuse(pixel, quarter, depth, 0.0, np.inf, 1.0)["values"][:, :1], [[F32(1.0) / F32(3.0)]])
    assert _same(R.fuse(pixel, quarter, depth[:, ::-1], 0.0, np.inf, 1.0)["values"][:, :1], [[F32(1.0 + 2.0 ** -23) / F32(3.0)]])
    # two problems share the projection
    two = R.fuse(pixel, z, np.concatenate([F32([2.0, 0.875, 0.0]).reshape(1, 3, 1, 1), np.zeros((1, 3, 1, 1), F32)]), 0.0, np.inf, 0.25)
    assert two["known"].tolist() == [3, 0] and _same(two["values"][0], fresh["values"][0]) and np.isnan(two["values"][1]).all()


# ---- the rule of the sampler ----------------------------------------------------------------------------------------------------------------
ORIGIN, STEP, DIMS = (0.0, -1.0, 2.0), (0.5, 0.25, 0.125), (2, 3, 4)


def _linear_field(dims=DIMS, origin=ORIGIN, step=STEP):
    """v = 2 x - y + 4 z on the nodes: dyadic, so the interpolant and its derivative (2, -1, 4) are exact."""
    p = R.node_points(origin, step, dims)
    return (2 * p[:, 0] - p[:, 1] + 4 * p[:, 2]).astype(F32)[None], np.ones((1, R.num_nodes(dims)), F32)


def test_a_row_on_the_last_node_plane_and_one_an_ulp_outside():
    values, weight = _linear_field()
    last = F32([0.5, -0.5, 2.375])                                          # node (1, 2, 3): g_c == dims - 1 on every axis
    pts = F32([last, [0.25, -0.875, 2.0625], [0.0, -1.0, 2.0], [-0.0, -1.0, 2.0],
               [up(0.5), -0.5, 2.375], [0.5, up(up(-0.5)), 2.375], [0.5, -0.5, up(2.375)],
               [down(0.0), -1.0, 2.0], [0.0, down(-1.0), 2.0], [0.0, -1.0, down(2.0)], [np.nan, -1.0, 2.0], [0.25, np.inf, 2.0]])
    got = R.sample(pts, ORIGIN, STEP, DIMS, values, weight)
    assert got["state"].tolist() == [[R.KNOWN] * 4 + [R.OUTSIDE] * 8] and got["states"].tolist() == [[8, 0, 4]]
    want = (2 * pts[:4, 0] - pts[:4, 1] + 4 * pts[:4, 2]).astype(F32)
    assert _same(got["distance"][0, :4], want) and _same(got["gradient"][0, :4], [[2.0, -1.0, 4.0]] * 4)
    assert np.isnan(got["distance"][0, 4:]).all() and np.isnan(got["gradient"][0, 4:]).all()
    # the rule is on g_c, not on x_c: one ulp above -0.5 is half an ulp of x - origin = 0.5 and rounds back onto the plane
    on = R.sample(F32([[0.5, up(-0.5), 2.375]]), ORIGIN, STEP, DIMS, values, weight)
    assert on["state"].tolist() == [[R.KNOWN]] and _same(on["distance"], want[:1][None])
    # the last plane uses the clamped cell with f == 1: the value is the far corner's even when the near corners hold anything
    values[0, : R.num_nodes(DIMS) - 1] = 99.0
    assert R.sample(last[None], ORIGIN, STEP, DIMS, values, weight)["distance"].tolist() == [[float(2 * 0.5 + 0.5 + 4 * 2.375)]]


def test_unknown_from_a_single_corner_without_a_weight_and_rows_that_are_not_read():
    values, weight = _linear_field()
    weight[0, (0 * 3 + 1) * 4 + 2] = 0.0                                     # node (0, 1, 2): a corner of the four cells around it
    values[0, (0 * 3 + 1) * 4 + 2] = NAN
    centres = F32([[0.25, -0.875 + 0.25 * j, 2.0625 + 0.125 * k] for j in range(2) for k in range(3)])
    got = R.sample(centres, ORIGIN, STEP, DIMS, values, weight)
    assert got["state"].tolist() == [[R.KNOWN, R.UNKNOWN, R.UNKNOWN, R.KNOWN, R.UNKNOWN, R.UNKNOWN]]
    assert got["states"].tolist() == [[0, 4, 2]] and np.isnan(got["distance"][0, [1, 2, 4, 5]]).all()
    assert np.isnan(got["gradient"][0, [1, 2, 4, 5]]).all() and _same(got["gradient"][0, [0, 3]], [[2.0, -1.0, 4.0]] * 2)
    # a weight that is not 0 counts, whatever it is; count and labels take rows out; one field for two point sets
    weight[0, 0] = 0.5
    labels = np.int32([0, 0, 0, -1, 0, 0])
    two = R.sample(np.stack([centres, centres[::-1]]), ORIGIN, STEP, DIMS, values, weight, count=5, labels=labels)
    assert two["state"].tolist() == [[2, 1, 1, 0, 1, 0], [1, 1, 2, 0, 1, 0]] and two["states"].tolist() == [[2, 3, 1]] * 2
    # a trilinear field that is not linear: the formulas by hand in one cell of unit steps, corner values C[a][b][c] = 1 + 4 a + 2 b + c + 8 a b c
    C = np.arange(1.0, 9.0, dtype=F32).reshape(2, 2, 2)
    C[1, 1, 1] += 8.0
    got = R.sample(F32([[0.5, 0.25, 0.75]]), (0, 0, 0), (1, 1, 1), (2, 2, 2), C.reshape(1, 8), np.ones((1, 8), F32))
    fx, fy, fz = 0.5, 0.25, 0.75
    assert got["distance"].tolist() == [[1 + 4 * fx + 2 * fy + fz + 8 * fx * fy * fz]]
    assert got["gradient"].tolist() == [[[4 + 8 * fy * fz, 2 + 8 * fx * fz, 1 + 8 * fx * fy]]]


# ---- the two methods of a sample, on the CPU ------------------------------------------------------------------------------------------------
def _clearance(state, distance, gradient):
    from neural_jacobian_field_amd.field_volume import FieldClearance
    state = torch.tensor(state, dtype=torch.int32)
    return FieldClearance(state=state, distance=torch.tensor(distance, dtype=torch.float32),
                          gradient=torch.tensor(gradient, dtype=torch.float32),
                          states=torch.stack([(state == c).sum(dim=1) for c in range(3)], dim=1).to(torch.int32))


def test_cost_with_and_without_known_rows():
    nan = float("nan")
    c = _clearance([[2, 2, 1, 0], [0, 1, 1, 0], [2, 0, 0, 0]], [[0.5, -0.25, nan, nan], [nan] * 4, [-3.0, nan, nan, nan]],
                   np.zeros((3, 4, 3)))
    got = c.cost()
    assert got.dtype == torch.float64 and got.shape == (3,) and got[0] == 0.375 and torch.isnan(got[1]) and got[2] == 3.0
    want = R.cost(c.state.numpy(), c.distance.numpy())
    assert np.array_equal(got.numpy(), want, equal_nan=True)


def test_surface_targets_with_a_zero_gradient():
    from neural_jacobian_field_amd.field_volume import INFORMATION_FLOOR
    nan = float("nan")
    pts = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]])
    c = _clearance([[2, 2, 1, 0]], [[0.5, 0.5, nan, nan]], [[[0.0, 0.0, -2.0], [0.0, 0.0, 0.0], [nan] * 3, [nan] * 3]])
    targets, information = c.surface_targets(pts)
    assert targets.shape == (1, 4, 3) and information.shape == (1, 4, 6) and targets.dtype == information.dtype == torch.float32
    assert targets[0, 0].tolist() == [1.0, 2.0, 3.25]                        # x - d g / (g . g): 0.5 at a slope of 2 is 0.25 away
    f = INFORMATION_FLOOR
    assert information[0, 0].tolist() == pytest.approx([f, 0, 0, f, 0, 1.0], abs=1e-12)
    assert torch.isnan(targets[0, 1:]).all() and torch.isnan(information[0, 1:]).all()      # g . g == 0, UNKNOWN, OUTSIDE
    want, normals = R.surface_targets(pts.numpy()[None], c.state.numpy(), c.distance.numpy(), c.gradient.numpy())
    assert np.array_equal(targets.numpy().astype(np.float64), want, equal_nan=True) and normals[0, 0].tolist() == [0.0, 0.0, -1.0]
    assert c.surface_targets(pts[None])[0].shape == (1, 4, 3)
    for bad in (None, pts.double(), pts[:3], pts[:, :2], pts.expand(2, 4, 3), pts.numpy()):
        with pytest.raises(ValueError, match="FieldClearance.surface_targets: points must be fp32 \\[4, 3\\] or \\[Mq, 4, 3\\] with Mq 1 or 1"):
            c.surface_targets(bad)


# ---- the interface --------------------------------------------------------------------------------------------------------------------------
def test_the_signatures():
    from neural_jacobian_field_amd import field_volume as fv
    from neural_jacobian_field_amd import hip
    params = inspect.signature(fv.fuse_depth).parameters
    assert list(params) == ["grid", "depth", "view", "truncation", "far", "max_weight", "into"]
    keywords = dict(far=float("inf"), max_weight=float("inf"), into=None)
    assert {k: params[k].default for k in keywords} == keywords
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    assert all(params[k].default is inspect.Parameter.empty for k in ("grid", "depth", "view", "truncation"))
    params = inspect.signature(fv.sample_distance).parameters
    assert list(params) == ["points", "field", "labels", "count"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None for k in ("labels", "count"))
    assert list(fv.FieldDistance.__dataclass_fields__) == ["grid", "truncation", "values", "weight", "known"]
    assert list(fv.FieldClearance.__dataclass_fields__) == ["state", "distance", "gradient", "states"] == list(R.SAMPLE_OUT)
    assert [name for name, _ in hip.FIELD_TSDF_OUTPUTS] == list(R.OUT)
    assert [name for name, _ in hip.FIELD_TSDF_SAMPLE_OUTPUTS] == list(R.SAMPLE_OUT)
    assert list(inspect.signature(fv.FieldDistance.mesh).parameters) == ["self", "capacities"]
    assert list(inspect.signature(fv.FieldClearance.cost).parameters) == ["self"]
    assert list(inspect.signature(fv.FieldClearance.surface_targets).parameters) == ["self", "points"]
    assert hip.FIELD_TSDF_STATE_NAMES == ("outside", "unknown", "known")
    assert (hip.FIELD_TSDF_OUTSIDE, hip.FIELD_TSDF_UNKNOWN, hip.FIELD_TSDF_KNOWN) == (R.OUTSIDE, R.UNKNOWN, R.KNOWN) == (0, 1, 2)


def _grid(dims=(5, 4, 3), step=(0.5, 0.5, 0.5)):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid((0.0, 0.0, 0.0), step, dims)


def test_fuse_depth_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldDistance, fuse_depth
    grid, depth = _grid(), torch.zeros(2, 1, 48, 64)

    def go(grid=grid, depth=depth, view=DEFAULT, truncation=0.1, **kw):
        return fuse_depth(grid, depth, _view() if view is DEFAULT else view, truncation, **kw)

    for bad in (None, (5, 4, 3), grid.c_grid()):
        with pytest.raises(ValueError, match="fuse_depth: grid must be a FieldGrid"):
            go(grid=bad)
    for bad in (None, depth.double(), depth[0, 0], depth[None], depth.numpy()):
        with pytest.raises(ValueError, match="fuse_depth: depth must be fp32 \\[V, H, W\\] or \\[M, V, H, W\\]"):
            go(depth=bad)
    for bad in (torch.zeros(0, 1, 48, 64), torch.zeros(1, 1, 1, 1).expand(65536, 1, 48, 64)):
        with pytest.raises(ValueError, match="fuse_depth: 1 to 65535 problems"):
            go(depth=bad)
    for bad in (None, dict(height=48)):
        with pytest.raises(ValueError, match="fuse_depth: the view must be a FieldView"):
            go(view=bad)
    for pattern, bad in _bad_views():
        if not pattern.startswith(("footprint", "tolerance")):                # the two fields of the z-buffer are not read
            with pytest.raises(ValueError, match="fuse_depth: " + pattern):
                go(view=bad)
    for bad in (torch.zeros(2, 2, 48, 64), torch.zeros(1, 48, 32), torch.zeros(2, 1, 64, 48)):
        with pytest.raises(ValueError, match="fuse_depth: depth must hold \\[1, 48, 64\\] images"):
            go(depth=bad)
    for bad in (0.0, -0.1, float("nan"), float("inf"), 1e39, 1e-50, None, True, "0.1"):
        with pytest.raises(ValueError, match="fuse_depth: truncation must be a finite number > 0"):
            go(truncation=bad)
    for bad in (0.0, -1.0, float("nan"), None, False, "4"):
        with pytest.raises(ValueError, match="fuse_depth: max_weight must be a number > 0"):
            go(max_weight=bad)
    for bad in (float("nan"), None, True, "2", 0.0, -1.0):
        with pytest.raises(ValueError, match="fuse_depth: far must be a number > near"):
            go(far=bad)
    with pytest.raises(ValueError, match="fuse_depth: far must be a number > near"):
        go(far=0.5, view=_view(near=0.5))
    with pytest.raises(ValueError, match="fuse_depth: M \\* nodes must stay below 2\\*\\*31"):
        go(grid=_grid((1024, 1024, 1024)), depth=depth)
    n = grid.num_nodes
    fine = dict(grid=grid, truncation=float(F32(0.1)), values=torch.zeros(2, n), weight=torch.zeros(2, n), known=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="fuse_depth: into must be a FieldDistance"):
        go(into=fine)
    for change in (dict(grid=_grid((5, 4, 4))), dict(grid=_grid(step=(0.5, 0.5, 0.25))), dict(truncation=0.2), dict(truncation=0.1)):
        with pytest.raises(ValueError, match="fuse_depth: into must be of the same grid and truncation"):
            go(into=FieldDistance(**{**fine, **change}))
    for what, bad in (("values", torch.zeros(1, n)), ("values", torch.zeros(2, n).double()), ("values", torch.zeros(n, 2).t()),
                      ("weight", torch.zeros(2, n + 1)), ("weight", None), ("known", torch.zeros(2)), ("known", torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(ValueError, match=f"fuse_depth: into.{what} must be a contiguous"):
            go(into=FieldDistance(**{**fine, what: bad}))
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="fuse_depth: intrinsics must live on the device of depth"):
            go(depth=depth.cuda())
        view = _view()
        view.intrinsics, view.cam2world = view.intrinsics.cuda(), view.cam2world.cuda()
        with pytest.raises(ValueError, match="fuse_depth: into.values must live on the device of depth"):
            go(depth=depth.cuda(), view=view, into=FieldDistance(**fine))
    # a view that visible_rows refuses for its z-buffer fields is fine here
    for kw in ({}, dict(depth=depth[0]), dict(view=_view(footprint=9, tolerance=-1.0, near=0.5), far=0.75, max_weight=1),
               dict(into=FieldDistance(**fine), max_weight=64.0, far=float("inf"))):
        with pytest.raises(ValueError, match="fuse_depth: .*no CPU path"):
            go(**kw)


def test_sample_distance_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldDistance, sample_distance
    grid, pts = _grid(), torch.zeros(2, 40, 3)
    n = grid.num_nodes

    def field(m=1, **kw):
        args = dict(grid=grid, truncation=0.1, values=torch.zeros(m, n), weight=torch.zeros(m, n), known=torch.zeros(m, dtype=torch.int32))
        args.update(kw)
        return FieldDistance(**args)

    for bad in (None, pts.double(), pts[..., :2], pts[0, 0], np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="sample_distance: points must be fp32 \\[n, 3\\] or \\[Mq, n, 3\\]"):
            sample_distance(bad, field())
    for bad in (None, torch.zeros(1, n), dict(values=torch.zeros(1, n)), field(grid=(5, 4, 3))):
        with pytest.raises(ValueError, match="sample_distance: field must be a FieldDistance"):
            sample_distance(pts, bad)
    for bad in (_grid((1, 4, 3)), _grid((5, 4, 1)), _grid(step=(0.5, 0.0, 0.5)), _grid(step=(0.5, 0.5, -0.5)), _grid(step=(float("inf"), 1, 1)),
                _grid(step=(float("nan"), 1, 1))):
        with pytest.raises(ValueError, match="sample_distance: the field's grid needs two nodes or more and a finite step > 0 on every axis"):
            sample_distance(pts, field(grid=bad, values=torch.zeros(1, bad.num_nodes), weight=torch.zeros(1, bad.num_nodes)))
    for what, bad in (("values", torch.zeros(1, n + 1)), ("values", torch.zeros(n)), ("weight", torch.zeros(1, n).double()), ("weight", None)):
        with pytest.raises(ValueError, match=f"sample_distance: field.{what} must be fp32 \\[Mf, {n}\\]"):
            sample_distance(pts, field(**{what: bad}))
    with pytest.raises(ValueError, match="sample_distance: field.values and field.weight must hold the same problems"):
        sample_distance(pts, field(weight=torch.zeros(2, n)))
    for points, f in ((torch.zeros(0, 40, 3), field()), (torch.zeros(65536, 1, 3), field()), (pts, field(0))):
        with pytest.raises(ValueError, match="sample_distance: 1 to 65535 problems"):
            sample_distance(points, f)
    for points, f in ((pts, field(3)), (torch.zeros(3, 40, 3), field(2))):
        with pytest.raises(ValueError, match="sample_distance: field and points hold one set or one per problem"):
            sample_distance(points, f)
    with pytest.raises(ValueError, match="sample_distance: M \\* n must stay below 2\\*\\*31"):
        sample_distance(torch.zeros(1, 3).expand(2 ** 15, 2 ** 16, 3), field())
    for bad in (3, torch.ones(2, dtype=torch.int32), torch.ones(1)):
        with pytest.raises(ValueError, match="sample_distance: count must be one int32"):
            sample_distance(pts, field(), count=bad)
    for bad in (torch.zeros(40), torch.zeros(39, dtype=torch.int32), [0] * 40):
        with pytest.raises(ValueError, match="sample_distance: labels must be int32 \\[40\\]"):
            sample_distance(pts, field(), labels=bad)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="sample_distance: field.values must live on the device of points"):
            sample_distance(pts.cuda(), field())
        with pytest.raises(ValueError, match="sample_distance: labels must live on the device of points"):
            sample_distance(pts.cuda(), field(values=torch.zeros(1, n).cuda(), weight=torch.zeros(1, n).cuda()),
                            labels=torch.zeros(40, dtype=torch.int32))
    for points, f, kw in ((pts, field(), {}), (pts[0], field(2), {}),
                          (pts, field(2), dict(count=torch.ones(1, dtype=torch.int32), labels=torch.zeros(40, dtype=torch.int32)))):
        with pytest.raises(ValueError, match="sample_distance: .*no CPU path"):
            sample_distance(points, f, **kw)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
ARGUMENTS = dict(njf_field_tsdf=18, njf_field_tsdf_sample=15)


def test_the_symbols_are_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count in ARGUMENTS.items():
        assert name in declared and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
        params = re.search(name + r"\s*\((.*?)\);", flat, flags=re.S).group(1)
        assert len(params.split(",")) == len(getattr(lib, name).argtypes) == count, name
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_TSDF_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_TSDF_STATES"] == hip.FIELD_TSDF_STATES == R.STATES == 3
    assert [defines[f"NJF_FIELD_TSDF_{n.upper()}"] for n in hip.FIELD_TSDF_STATE_NAMES] == [0, 1, 2]


def _c_grid(dims=(5, 4, 3), step=(0.5, 0.5, 0.5), origin=(0.0, 0.0, 0.0)):
    from neural_jacobian_field_amd import hip
    return hip.make_field_grid(origin, step, dims)


def test_the_fusion_entry_refuses_bad_arguments_without_a_gpu(lib):
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("grid", "depth", "num_problems", "views", "height", "width", "k", "w2c", "near", "far", "truncation", "max_weight",
             "values_in", "weight_in", "values", "weight", "known")

    def call(**kw):
        args = {k: P for k in names}
        args.update(grid=_c_grid(), num_problems=3, views=2, height=0, width=64, near=0.0, far=float("inf"), truncation=0.1,
                    max_weight=float("inf"))
        args.update(kw)
        grid = args.pop("grid")
        return lib.njf_field_tsdf(None if grid is None else C.byref(grid), *[args[k] for k in names[1:]], None)

    # every call that could pass its other checks keeps height = 0, so that none reaches a launch
    assert call() == E_SHAPE
    for key in ("grid", "depth", "k", "w2c", "values", "weight", "known"):
        assert call(**{key: None}) == E_NULL, key
        assert call(**{key: None}, views=0) == E_NULL, key                            # a missing pointer is judged first
    assert call(values_in=None) == E_NULL and call(weight_in=None) == E_NULL          # one of the pair without the other
    assert call(values_in=None, weight_in=None) == E_SHAPE
    for key, values in (("num_problems", (0, -1, 65536)), ("views", (0, -1, 33)), ("near", (-1.0, float("nan"), float("inf"))),
                        ("far", (0.0, -1.0, float("nan"))), ("truncation", (0.0, -0.1, float("nan"), float("inf"))),
                        ("max_weight", (0.0, -1.0, float("nan")))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)                          # (judged before the shapes)
    assert call(near=0.5, far=0.5) == E_VALUE and call(near=0.5, far=0.75, max_weight=1.0, views=32, num_problems=65535) == E_SHAPE
    for kw in (dict(height=-1), dict(height=4, width=0), dict(height=4, grid=_c_grid((0, 4, 3))), dict(height=4, grid=_c_grid((5, -1, 3))),
               dict(height=4, grid=_c_grid((2048, 1024, 1024))), dict(height=4, grid=_c_grid((1024, 1024, 1024))),
               dict(height=2 ** 16, width=2 ** 15), dict(height=2 ** 14, width=2 ** 14, num_problems=3, views=3),
               dict(height=4, num_problems=2, grid=_c_grid((1024, 1024, 1024)))):
        assert call(**kw) == E_SHAPE, kw


def test_the_sampling_entry_refuses_bad_arguments_without_a_gpu(lib):
    P = 0x1000
    names = ("points", "count", "labels", "num_queries", "n", "num_problems", "grid", "values", "weight", "num_fields", "state", "distance",
             "gradient", "states")

    def call(**kw):
        args = {k: P for k in names}
        args.update(num_queries=3, n=-1, num_problems=3, grid=_c_grid(), num_fields=3)
        args.update(kw)
        args["grid"] = None if args["grid"] is None else C.byref(args["grid"])
        return lib.njf_field_tsdf_sample(*[args[k] for k in names], None)

    # every call that could pass its other checks keeps n = -1, so that none reaches a launch
    assert call() == E_SHAPE
    for key in ("points", "grid", "values", "weight", "state", "distance", "gradient", "states"):
        assert call(**{key: None}) == E_NULL, key
        assert call(**{key: None}, num_problems=0) == E_NULL, key
    assert call(count=None, labels=None) == E_SHAPE                                   # the two optional inputs
    for key, values in (("num_problems", (0, -1, 65536)), ("num_queries", (0, 2, 4, -3)), ("num_fields", (0, 2, 4, -3))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)
    assert call(num_queries=1, num_fields=1) == E_SHAPE and call(num_queries=1) == E_SHAPE and call(num_fields=1) == E_SHAPE
    for bad in (_c_grid((1, 4, 3)), _c_grid((5, 1, 3)), _c_grid((5, 4, 1)), _c_grid(step=(0.0, 0.5, 0.5)), _c_grid(step=(0.5, -0.5, 0.5)),
                _c_grid(step=(0.5, 0.5, float("nan"))), _c_grid(step=(float("inf"), 0.5, 0.5)), _c_grid(origin=(0.0, float("inf"), 0.0)),
                _c_grid(origin=(float("nan"), 0.0, 0.0))):
        assert call(grid=bad) == E_VALUE
    for kw in (dict(grid=_c_grid((0, 4, 3))), dict(grid=_c_grid((5, 4, -2))), dict(grid=_c_grid((2048, 1024, 1024))),
               dict(n=0, grid=_c_grid((1024, 1024, 1024))), dict(n=2 ** 30, num_problems=2, num_queries=2, num_fields=1),
               dict(n=0, num_problems=2, num_queries=1, num_fields=2, grid=_c_grid((1024, 1024, 1024)))):
        assert call(**kw) == E_SHAPE, kw


# ---- the condition of the GPU's end-to-end test, on the CPU ---------------------------------------------------------------------------------
def e2e_commands(planted):
    """The five commands of section 26 table (c): the planted one, zero and three others."""
    return (tuple(float(v) for v in planted[0]), (0.0, 0.0, 0.0)) + COMMANDS


def e2e_poses(s, planted):
    """fp32 [5, 878, 3]: the shell of the section-22 scene at the five commands."""
    return np.stack([F.posed_targets(s["twists"], np.float32([u]), s["xyz"], s["labels"], s["parts"], s["joints"], s["tree"])[0]
                     for u in e2e_commands(planted)]).astype(F32)


def test_the_planted_command_has_the_smallest_cost_in_the_fused_frame():
    s, k, c2w, planted, depth, _ = section_22_scene()
    poses = e2e_poses(s, planted)
    lower, upper = np.float64(E2E_ORIGIN), np.float64(E2E_ORIGIN) + (np.float64(E2E_DIMS) - 1) * np.float64(E2E_STEP)
    assert (poses.min(axis=(0, 1)) > lower).all() and (poses.max(axis=(0, 1)) < upper).all()      # no pose leaves the grid
    field = R.fuse_depth(E2E_ORIGIN, E2E_STEP, E2E_DIMS, depth[None], k, c2w, 0.0, np.inf, E2E_TRUNCATION)
    got = R.sample(poses, E2E_ORIGIN, E2E_STEP, E2E_DIMS, field["values"], field["weight"])
    cost = R.cost(got["state"], got["distance"])
    print("known nodes", field["known"].tolist(), "states", got["states"].tolist(), "cost", [f"{c:.4e}" for c in cost],
          f"margin {cost[1:].min() - cost[0]:.3e}")
    assert field["known"].tolist() == [4238] and (got["states"][:, R.OUTSIDE] == 0).all() and (got["states"].sum(axis=1) == 878).all()
    assert all(cost[0] < c for c in cost[1:])                          # the condition the GPU test relies on
    assert np.allclose(cost, E2E_COST, rtol=0, atol=5e-6)              # the figures of DESIGN.md section 27
    assert abs((cost[1:].min() - cost[0]) - 3.50e-3) < 1e-5
