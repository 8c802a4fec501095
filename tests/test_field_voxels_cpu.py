"""Host-side tests of the observed clouds from depth images (field_volume.depth_points / voxel_reduce; njf_field_depth_points,
njf_field_voxels): the numpy restatement (tests/field_voxels_restatement.py) -- the integer sums do not
depend on the order of the points, the centroid stays within the header's bound of the float64 mean, the inside rule at the
faces of the lattice, min_points, capacity, count, non-finite rows; the depth mask written out by hand and a pinhole model
against get_pixel_coordinates --, every argument check of both functions, raised before any device work (there is no GPU
here), and the C ABI's symbols and return codes."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_voxels_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


def _lattice(rng, dims_max=1024):
    """A random lattice: 1 to dims_max cells per axis (log-uniform), cells from 1e-3 to 10, an origin of either sign."""
    dims = tuple(int(round(2 ** rng.uniform(0, np.log2(dims_max)))) for _ in range(3))
    cell = float(F32(10 ** rng.uniform(-3, 1)))
    origin = tuple(float(F32(v)) for v in rng.uniform(-5, 5, 3) * cell * max(dims) ** rng.uniform(0, 1))
    return origin, cell, dims


# ---- (i) the integer sums and the centroid ----------------------------------------------------------------------------------------------
def test_the_sums_do_not_depend_on_the_order_of_the_points():
    rng = np.random.default_rng(22)
    origin, cell, dims = (-0.3, 0.1, 2.0), 0.05, (6, 5, 4)
    pts = (np.asarray(origin) + rng.uniform(-0.1, 1.1, (3000, 3)) * np.asarray(dims) * cell).astype(F32)
    pts[:40] = pts[40]                                          # coincident points
    first = S.voxels(pts[None], origin, cell, dims)
    assert first["count"][0] > 100 and first["outside"][0] > 100 and first["weight"].max() > 20
    for _ in range(20):
        again = S.voxels(pts[rng.permutation(pts.shape[0])][None], origin, cell, dims)
        for key in first:
            assert again[key].dtype == first[key].dtype and again[key].tobytes() == first[key].tobytes(), key
    assert first["sums"].dtype == np.int64 and first["sums"].min() >= 0
    assert (first["sums"] <= first["weight"][..., None].astype(np.int64) * S.QUANTUM).all()


def test_the_centroid_stays_within_the_bound_of_the_float64_mean():
    rng = np.random.default_rng(122)
    worst = 0.0
    for case in range(200):
        origin, cell, dims = _lattice(rng)
        n = 400
        cells = np.stack([rng.integers(0, d, 12) for d in dims], axis=-1)            # a dozen cells, ~33 points in each
        pts = (np.asarray(origin, dtype=np.float64) + (cells[rng.integers(0, 12, n)] + rng.uniform(0, 1, (n, 3))) * cell).astype(F32)
        got = S.voxels(pts[None], origin, cell, dims)
        valid, inside, index, _ = S.classify(pts, origin, cell, dims)
        t_abs = np.abs(S.cell_coordinates(pts, origin, cell).astype(np.float64))
        kept = int(got["count"][0])
        assert kept >= 1 and got["outside"][0] + got["weight"][0].sum() == n
        for row in range(kept):
            members = inside & (index == got["cell"][0, row])
            assert members.sum() == got["weight"][0, row]
            mean = pts[members].astype(np.float64).mean(axis=0)
            bound = S.mean_bound(got["points"][0, row].astype(np.float64), t_abs[members].max(axis=0), cell)
            worst = max(worst, float((np.abs(got["points"][0, row].astype(np.float64) - mean) / bound).max()))
    print(f"largest |centroid - float64 mean| / bound over 200 lattices: {worst:.3f}")
    assert worst <= 1.0


# ---- (ii) the inside rule -----------------------------------------------------------------------------------------------------------------
def test_the_inside_rule_at_the_faces_of_the_lattice():
    origin, cell, dims = (0.5, -1.0, 0.25), 0.25, (4, 3, 2)
    upper = [o + d * cell for o, d in zip(origin, dims)]                             # exact in fp32
    below = float(np.nextafter(F32(origin[0]), F32(-np.inf)))
    pts = F32([[origin[0], origin[1], origin[2]],                                    # the lower corner: inside, cell 0, q = 0
               [upper[0], -0.9, 0.3],                                                # exactly on the upper x face: outside
               [float(np.nextafter(F32(upper[0]), F32(-np.inf))), -0.9, 0.3],        # one ulp below it: inside, the last x cell
               [below, -0.9, 0.3],                                                   # one ulp below the origin: outside
               [0.6, upper[1], 0.3], [0.6, -0.9, upper[2]],                          # the other two upper faces: outside
               [0.6, -0.9, 0.3]])
    valid, inside, index, q = S.classify(pts, origin, cell, dims)
    assert valid.all() and inside.tolist() == [True, False, True, False, False, False, True]
    assert index[0] == 0 and q[0].tolist() == [0, 0, 0]
    assert index[2] == (3 * 3 + 0) * 2 + 0 and q[2, 0] == S.QUANTUM                   # the fraction rounds up to one whole cell
    out = S.voxels(pts[None], origin, cell, dims)
    assert out["outside"][0] == 4 and out["count"][0] == 2 and out["cell"][0, :3].tolist() == [0, 18, -1]
    assert out["weight"][0, :3].tolist() == [2, 1, 0]                               # the corner and the plain point share cell 0
    # dims of 1 on every axis: one cell, everything in [origin, origin + cell) lands in it
    one = S.voxels(F32([[[0.5, -1.0, 0.25], [0.7, -0.8, 0.45], [0.75, -0.8, 0.45], [0.49, -0.8, 0.45]]]), origin, cell, (1, 1, 1))
    assert one["count"][0] == 1 and one["weight"][0, 0] == 2 and one["outside"][0] == 2 and one["points"].shape == (1, 1, 3)
    assert np.allclose(one["points"][0, 0], [0.6, -0.9, 0.35], atol=1e-6)


def test_points_far_outside_the_lattice_are_counted_and_not_reduced():
    rng = np.random.default_rng(5)
    origin, cell, dims = (0.0, 0.0, 0.0), 0.1, (10, 10, 10)
    pts = rng.uniform(-0.4, 1.4, (2000, 3)).astype(F32)                              # 40 % beyond the box on every side
    out = S.voxels(pts[None], origin, cell, dims)
    box = ((pts >= 0) & (pts < 1)).all(axis=-1)
    assert abs(int(out["outside"][0]) - int((~box).sum())) <= 2                      # (up to a point within an ulp of a face)
    assert out["weight"].sum() + out["outside"][0] == 2000
    n = int(out["count"][0])
    assert (out["points"][0, :n] >= 0).all() and (out["points"][0, :n] <= 1).all()    # no centroid outside the lattice
    huge = S.voxels(F32([[[3e38, 0.5, 0.5], [-3e38, 0.5, 0.5], [0.55, 0.55, 0.55]]]), origin, cell, dims)
    assert huge["outside"][0] == 2 and huge["count"][0] == 1 and huge["cell"][0, 0] == 555


# ---- (iii) min_points, capacity, count, non-finite rows ---------------------------------------------------------------------------------
def _speckled():
    rng = np.random.default_rng(7)
    origin, cell, dims = (0.0, 0.0, 0.0), 0.25, (4, 4, 4)
    dense = (F32([0.3, 0.3, 0.3]) + rng.uniform(0, 0.2, (30, 3))).astype(F32)          # one cell
    lone = F32([[0.9, 0.1, 0.1], [0.1, 0.9, 0.6], [0.6, 0.6, 0.9]])                   # three cells of one point
    pair = F32([[0.8, 0.8, 0.1], [0.85, 0.85, 0.15]])
    return origin, cell, dims, np.concatenate([lone[:1], dense, pair, lone[1:]])[None]


def test_min_points_removes_speckle():
    origin, cell, dims, pts = _speckled()
    assert S.voxels(pts, origin, cell, dims)["count"][0] == 5
    two = S.voxels(pts, origin, cell, dims, min_points=2)
    assert two["count"][0] == 2 and sorted(two["weight"][0, :2].tolist()) == [2, 30] and two["weight"][0, 2:].tolist() == [0] * 33
    assert S.voxels(pts, origin, cell, dims, min_points=31)["count"][0] == 0


def test_a_capacity_below_the_kept_count_keeps_the_first_cells_and_the_true_count():
    origin, cell, dims, pts = _speckled()
    full = S.voxels(pts, origin, cell, dims)
    assert (np.diff(full["cell"][0, :5]) > 0).all()                                  # ascending cell index
    for cap in (1, 4, 5, 9):
        cut = S.voxels(pts, origin, cell, dims, capacity=cap)
        n = min(cap, 5)
        assert cut["count"][0] == 5 and cut["points"].shape == (1, cap, 3)
        for key in ("points", "weight", "cell", "sums"):
            assert cut[key][0, :n].tobytes() == full[key][0, :n].tobytes(), key
        assert np.isnan(cut["points"][0, n:]).all() and (cut["weight"][0, n:] == 0).all() and (cut["cell"][0, n:] == -1).all()
        assert (cut["sums"][0, n:] == 0).all()


def test_non_finite_rows_and_rows_from_the_count_on_are_not_points():
    origin, cell, dims, pts = _speckled()
    dirty = np.concatenate([pts, F32([[[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf], [np.nan] * 3]])], axis=1)
    clean, got = S.voxels(pts, origin, cell, dims), S.voxels(dirty, origin, cell, dims)
    for key in ("count", "outside"):
        assert got[key].tobytes() == clean[key].tobytes()
    assert got["points"][0, :5].tobytes() == clean["points"][0, :5].tobytes()
    both = np.concatenate([pts, pts], axis=0)
    counted = S.voxels(both, origin, cell, dims, count=[31, 1000])
    assert counted["count"].tolist() == [2, 5] and counted["weight"][0, :2].tolist() == [30, 1]
    assert S.voxels(both, origin, cell, dims, count=[0, -3])["count"].tolist() == [0, 0]


# ---- (iv) the depth restatement -----------------------------------------------------------------------------------------------------------
def test_the_pinhole_model_uses_the_pixel_grid_of_get_pixel_coordinates():
    from neural_jacobian_field_amd.geometry import get_pixel_coordinates
    for h, w in ((1, 1), (3, 4), (5, 7)):
        xy, _ = get_pixel_coordinates(h, w)
        assert np.allclose(S.pixel_centres(h, w), xy.reshape(-1, 2).double().numpy(), atol=1e-7)
    # a camera at (1, 2, 3) looking along world +x (camera z), camera x = world -y ... a rotation and a translation
    k = np.array([[[0.8, 0.0, 0.5], [0.0, 1.1, 0.5], [0.0, 0.0, 1.0]]])
    c2w = np.array([[[0.0, 0.0, 1.0, 1.0], [-1.0, 0.0, 0.0, 2.0], [0.0, -1.0, 0.0, 3.0], [0.0, 0.0, 0.0, 1.0]]])
    depth = np.full((1, 3, 4), 2.0)
    z = S.pinhole_points(depth, k, c2w, "z")
    ray = S.pinhole_points(depth, k, c2w, "ray")
    assert np.allclose(z[0, :, 0], 1.0 + 2.0)                                        # z depth 2: the plane x = 3 in the world
    assert np.allclose(np.linalg.norm(ray[0] - [1.0, 2.0, 3.0], axis=-1), 2.0)        # ray depth 2: the sphere of radius 2
    # the same pixel, both kinds, lie on one ray through the camera centre
    a, b = z[0] - [1.0, 2.0, 3.0], ray[0] - [1.0, 2.0, 3.0]
    assert np.allclose(np.cross(a, b), 0.0, atol=1e-12) and (np.einsum("ij,ij->i", a, b) > 0).all()
    # pixel (row 1, col 2) by hand: x = 2.5 / 4, y = 1.5 / 3; camera point ((x - 0.5) / 0.8, (y - 0.5) / 1.1, 1) * 2
    cam = np.array([(0.625 - 0.5) / 0.8, 0.0, 1.0]) * 2.0
    assert np.allclose(z[0, 1 * 4 + 2], [1.0 + cam[2], 2.0 - cam[0], 3.0 - cam[1]])


def test_the_flying_pixel_rule_written_out_by_hand():
    nan, inf = np.nan, np.inf
    depth = F32([[[1.00, 1.04, 2.00, 2.05],
                  [1.00, 0.00, 2.00, nan],
                  [1.02, 1.05, 1.09, 2.10]]])
    valid = S.depth_valid(depth)
    assert valid[0].tolist() == [[True, True, True, True], [True, False, True, False], [True, True, True, True]]
    # max_jump 0.1: an edge where |d - dn| > 0.1 * min(d, dn).  Row 0: 1.04 | 2.00 is an edge, both go.  Row 1: the zero and the
    # NaN are invalid and do not count as neighbours, so (1,0) stays although 0.00 is far from 1.00; (1,2) = 2.00 has the valid
    # neighbours 2.00 above and 1.09 below -- an edge -- and goes, with 1.09.  Row 2: 1.09 | 2.10 is an edge; (2,3) = 2.10 also
    # loses to 1.09 only -- above it is the NaN; (2,1) = 1.05 against 1.09 and 1.02: no edge, and above it the zero: stays.
    want = [[True, False, False, True], [True, False, False, False], [True, True, False, False]]
    assert S.depth_mask(depth, max_jump=0.1)[0].tolist() == want
    # the image border: a 1 x 1 image has no neighbour at all, a 1 x 2 image one
    assert S.depth_mask(F32([[[3.0]]]), max_jump=0.01).tolist() == [[[True]]]
    assert S.depth_mask(F32([[[3.0, 4.0]]]), max_jump=0.01).tolist() == [[[False, False]]]
    # near, far: near < d <= far; inf, negative and zero depths never pass
    d = F32([[[0.5, 1.0, 2.0, 2.5, inf, -1.0, 0.0, nan]]])
    assert S.depth_valid(d, near=0.5, far=2.0).tolist() == [[[False, True, True, False, False, False, False, False]]]
    assert S.depth_valid(d).tolist() == [[[True, True, True, True, False, False, False, False]]]
    # the rule is symmetric: the mask of the mirrored image is the mirrored mask
    assert S.depth_mask(depth[:, :, ::-1], max_jump=0.1)[0].tolist() == [row[::-1] for row in want]


# ---- (v) the Python entries check their arguments before any device work -----------------------------------------------------------------
def test_the_signatures():
    from neural_jacobian_field_amd import field_volume as fv
    p = inspect.signature(fv.depth_points).parameters
    assert list(p) == ["depth", "intrinsics", "cam2world", "kind", "near", "far", "max_jump", "views_per_scene"]
    assert [p[k].default for k in list(p)[3:]] == ["z", 0.0, float("inf"), None, 1]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[3:])
    p = inspect.signature(fv.voxel_reduce).parameters
    assert list(p) == ["points", "cells", "count", "min_points", "capacity"]
    assert [p[k].default for k in list(p)[2:]] == [None, 1, None]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
    assert list(fv.FieldDepthPoints.__dataclass_fields__) == ["points", "kept"]
    assert list(fv.FieldVoxels.__dataclass_fields__) == ["points", "weight", "cell", "sums", "count", "outside"]


def test_depth_points_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import depth_points
    d, k, c = torch.ones(2, 3, 4), torch.eye(3).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1)
    for bad in (None, d.double(), d[0], d[None], torch.ones(2, 0, 4), np.ones((2, 3, 4), dtype=np.float32)):
        with pytest.raises(ValueError, match="depth_points: depth must be fp32 \\[B, H, W\\]"):
            depth_points(bad, k, c)
    for bad in (None, k.double(), k[:1], torch.eye(4).repeat(2, 1, 1)):
        with pytest.raises(ValueError, match="depth_points: intrinsics must be fp32 \\[2, 3, 3\\]"):
            depth_points(d, bad, c)
    for bad in (None, c.double(), c[:1], c[:, :3]):
        with pytest.raises(ValueError, match="depth_points: cam2world must be fp32 \\[2, 4, 4\\]"):
            depth_points(d, k, bad)
    for bad in ("Z", "depth", None, 1):
        with pytest.raises(ValueError, match="depth_points: kind must be one of \\['ray', 'z'\\]"):
            depth_points(d, k, c, kind=bad)
    for key in ("near", "far"):
        for bad in (None, "1", True, float("nan")):
            with pytest.raises(ValueError, match=f"depth_points: {key} must be a number"):
                depth_points(d, k, c, **{key: bad})
    for near, far in ((-0.1, 1.0), (float("inf"), float("inf")), (1.0, 1.0), (2.0, 1.0), (0.0, 0.0), (0.0, 1e-60), (1e39, float("inf"))):
        with pytest.raises(ValueError, match="depth_points: 0 <= near < far"):
            depth_points(d, k, c, near=near, far=far)
    for bad in (0.0, -0.1, float("nan"), float("inf"), True, "0.1", 1e-60, 1e39):
        with pytest.raises(ValueError, match="depth_points: max_jump must be a finite number > 0 or None"):
            depth_points(d, k, c, max_jump=bad)
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="depth_points: views_per_scene must be an integer >= 1"):
            depth_points(d, k, c, views_per_scene=bad)
    with pytest.raises(ValueError, match="depth_points: the batch \\(2\\) must be a multiple of views_per_scene \\(3\\)"):
        depth_points(d, k, c, views_per_scene=3)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="depth_points: intrinsics must live on the device of depth"):
            depth_points(d.cuda(), k, c.cuda())
    for kw in ({}, dict(kind="ray", near=0.1, far=5.0, max_jump=0.05, views_per_scene=2), dict(near=1e-50)):
        with pytest.raises(ValueError, match="depth_points: .*no CPU path"):
            depth_points(d, k, c, **kw)


def test_voxel_reduce_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, cell_grid, voxel_reduce
    pts, cells = torch.zeros(2, 50, 3), cell_grid((0, 0, 0), (1, 1, 1), 0.25)
    for bad in (None, pts.double(), torch.zeros(50, 2), torch.zeros(2, 0, 3), torch.zeros(3)):
        with pytest.raises(ValueError, match="voxel_reduce: points must be fp32 \\[T, 3\\] or \\[Mo, T, 3\\]"):
            voxel_reduce(bad, cells)
    for bad in (None, (0, 0, 0), cells.c_grid()):
        with pytest.raises(ValueError, match="voxel_reduce: cells must be a FieldGrid"):
            voxel_reduce(pts, bad)
    with pytest.raises(ValueError, match="voxel_reduce: cells must have three equal steps > 0"):
        voxel_reduce(pts, FieldGrid((0, 0, 0), (0.1, 0.1, 0.2), (4, 4, 4)))
    with pytest.raises(ValueError, match="voxel_reduce: at most 1024 cells per axis"):
        voxel_reduce(pts, FieldGrid((0, 0, 0), (0.1, 0.1, 0.1), (4, 1025, 4)))
    with pytest.raises(ValueError, match="voxel_reduce: Mo \\* the number of cells must stay below 2\\*\\*31"):
        voxel_reduce(pts, FieldGrid((0, 0, 0), (0.1, 0.1, 0.1), (1024, 1024, 1024)))
    for bad in (torch.ones(3, dtype=torch.int32), torch.ones(2, dtype=torch.int64), [50, 50], 50):
        with pytest.raises(ValueError, match="voxel_reduce: count must be int32 \\[2\\]"):
            voxel_reduce(pts, cells, count=bad)
    for bad in (0, -1, 2 ** 31, 1.0, True, None):
        with pytest.raises(ValueError, match="voxel_reduce: min_points must be an integer in \\[1, 2\\*\\*31\\)"):
            voxel_reduce(pts, cells, min_points=bad)
    for bad in (0, -5, 2 ** 30, 1.0, True):
        with pytest.raises(ValueError, match="voxel_reduce: capacity must be an integer >= 1"):
            voxel_reduce(pts, cells, capacity=bad)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="voxel_reduce: count must live on the device of points"):
            voxel_reduce(pts.cuda(), cells, count=torch.ones(2, dtype=torch.int32))
    for args, kw in (((pts,), {}), ((pts[0],), {}), ((pts,), dict(count=torch.ones(2, dtype=torch.int32), min_points=3, capacity=7))):
        with pytest.raises(ValueError, match="voxel_reduce: .*no CPU path"):
            voxel_reduce(*args, cells, **kw)


def test_the_shared_checks_still_speak_for_their_callers():
    """``_check_nearest`` hands the cloud and the lattice to the helper ``voxel_reduce`` uses: same messages, same order."""
    from neural_jacobian_field_amd.field_volume import cell_grid, nearest_points
    q, cells = torch.zeros(10, 3), cell_grid((0, 0, 0), (1, 1, 1), 0.25)
    with pytest.raises(ValueError, match="nearest_points: observed must be fp32 \\[T, 3\\] or \\[Mo, T, 3\\] with T >= 1"):
        nearest_points(q, torch.zeros(0, 3), cells, 0.1)
    with pytest.raises(ValueError, match="nearest_points: cells must be a FieldGrid"):
        nearest_points(q, torch.zeros(5, 3), None, float("nan"))                      # the lattice is judged before the distance
    with pytest.raises(ValueError, match="nearest_points: observed_count must be int32 \\[1\\]"):
        nearest_points(q, torch.zeros(5, 3), cells, 0.1, observed_count=torch.ones(2, dtype=torch.int32))


def test_the_three_entries_refuse_the_same_lattices(lib):
    """One cell list stands behind njf_field_nearest, njf_field_normals and njf_field_voxels: a lattice
    that one of them refuses, all three refuse, with NJF_E_VALUE, whatever else the call holds."""
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    entries = (
        (lib.njf_field_nearest,
         ("observed", "observed_count", "clouds", "points", "queries", "count", "labels", "clouds", "n", "clouds", "cells", 0.5, "index",
          "distance2", "matched", "found", "workspace", "words", 3)),
        (lib.njf_field_normals,
         ("observed", "observed_count", "clouds", "points", "queries", "count", "clouds", "n", "clouds", "cells", 0.5, 3, "viewpoint",
          "clouds", "moments", "normal", "neighbours", "variation", "eigenvalues", "workspace", "words", 7)),
        (lib.njf_field_voxels,
         ("observed", "observed_count", "clouds", "points", "cells", 1, 720, "out_points", "weight", "cell_index", "sums", "count",
          "outside", "workspace", "words", 7)))

    def codes(origin=(0.0, 0.0, 0.0), step=(0.25, 0.25, 0.25), dims=(8, 9, 10), clouds=5, **kw):
        values = dict(clouds=clouds, points=5000, n=300, words=2 ** 62, cells=hip.make_field_grid(origin, step, dims))
        values.update(kw)
        return [entry(*[values.get(a, P) if isinstance(a, str) else a for a in args], None) for entry, args in entries]

    assert codes(workspace=None) == [E_NULL] * 3                 # the lattice of the table is good: only the workspace is missing
    nan, inf = float("nan"), float("inf")
    bad = [dict(step=s) for s in ((0.25, 0.25, 0.5), (0.25, 0.5, 0.25), (0.0,) * 3, (-0.25,) * 3, (nan,) * 3, (inf,) * 3, (1e-45,) * 3)]
    bad += [dict(dims=d) for d in ((0, 9, 10), (8, -1, 10), (8, 9, 1025), (1025, 9, 10))]
    bad += [dict(origin=o) for o in ((nan, 0.0, 0.0), (0.0, nan, 0.0), (0.0, 0.0, inf))]
    bad += [dict(dims=(1024, 1024, 1024), clouds=2)]             # Mo * C = 2^31
    for lattice in bad:
        assert codes(**lattice) == [E_VALUE] * 3, lattice
        assert codes(**lattice, workspace=None, points=0) == [E_VALUE] * 3, lattice   # (judged before the shapes and the pointers)
    assert codes(dims=(1024, 1024, 1023), clouds=2, workspace=None) == [E_NULL] * 3   # the largest list: 2^31 - 2^21 cells


# ---- (vi) the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for symbol, arguments in (("njf_field_depth_points", 14), ("njf_field_voxels", 17)):
        assert symbol in declared and symbol in hip.EXPORTED_SYMBOLS and hasattr(lib, symbol)
        params = re.search(symbol + r"\s*\((.*?)\);", flat, flags=re.S).group(1)
        assert len(params.split(",")) == len(getattr(lib, symbol).argtypes) == arguments
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_(?:VOXELS|DEPTH)_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_VOXELS_ALL"] == hip.FIELD_VOXELS_ALL == sum(hip.FIELD_VOXELS_PHASES) == 7
    assert [defines[f"NJF_FIELD_VOXELS_{n.upper()}"] for n in hip.FIELD_VOXELS_PHASE_NAMES] == list(hip.FIELD_VOXELS_PHASES)
    assert defines["NJF_FIELD_VOXELS_WAVE"] == hip.FIELD_VOXELS_WAVE == 8
    assert defines["NJF_FIELD_VOXELS_QUANTUM"] == hip.FIELD_VOXELS_QUANTUM == S.QUANTUM == 2 ** 20
    assert defines["NJF_FIELD_DEPTH_RAY"] == hip.FIELD_DEPTH_RAY == hip.FIELD_DEPTH_KINDS["ray"] == 0
    assert defines["NJF_FIELD_DEPTH_Z"] == hip.FIELD_DEPTH_Z == hip.FIELD_DEPTH_KINDS["z"] == 1
    assert "#define NJF_FIELD_VOXELS_WORKSPACE(M, C, T) (NJF_FIELD_NEAREST_WORKSPACE(M, C, T) + 8LL * (M) * (C) + 1LL)" in header
    assert hip.field_voxels_workspace(3, 1000, 77) == hip.field_nearest_workspace(3, 1000, 77) + 8 * 3 * 1000 + 1


def test_the_depth_entry_refuses_bad_arguments_without_a_gpu(lib):
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("depth", "batch", "height", "width", "k_inv", "c2w", "kind", "near", "far", "max_jump", "views_per_scene", "points", "kept")

    def call(**kw):
        args = {k: P for k in names}
        args.update(batch=4, height=48, width=64, kind=1, near=0.0, far=float("inf"), max_jump=0.0, views_per_scene=2)
        args.update(kw)
        return lib.njf_field_depth_points(*[args[k] for k in names], None)

    for key in ("depth", "k_inv", "c2w", "points", "kept"):
        assert call(**{key: None}) == E_NULL, key
    for kw in (dict(batch=0), dict(height=0), dict(width=-1), dict(batch=2 ** 11, height=2 ** 10, width=2 ** 10),
               dict(views_per_scene=0), dict(views_per_scene=3), dict(views_per_scene=-2)):
        assert call(**kw, depth=None) == E_NULL and call(**kw) == E_SHAPE, kw          # (the pointers are judged first)
    for kw in (dict(kind=2), dict(kind=-1), dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")), dict(far=float("nan")),
               dict(far=0.0), dict(near=2.0, far=2.0), dict(near=2.0, far=1.0), dict(max_jump=-0.5), dict(max_jump=float("nan")),
               dict(max_jump=float("inf"))):
        assert call(**kw) == E_VALUE, kw


def test_the_voxels_entry_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("points", "points_count", "num_problems", "num_points", "cells", "min_points", "capacity", "out_points", "weight",
             "cell_index", "sums", "count", "outside", "workspace", "workspace_words", "phases")
    need = hip.field_voxels_workspace(5, 8 * 9 * 10, 5000)

    def call(origin=(0.0, 0.0, 0.0), step=(0.25, 0.25, 0.25), dims=(8, 9, 10), **kw):
        args = {k: P for k in names}
        args.update(num_problems=5, num_points=5000, min_points=1, capacity=720, workspace_words=need, phases=7,
                    cells=hip.make_field_grid(origin, step, dims))
        args.update(kw)
        return lib.njf_field_voxels(*[args[k] for k in names], None)

    # every call that could pass its checks is given a missing pointer, so that none reaches a launch
    for key, values in (("num_problems", (0, -1, 65536)), ("phases", (0, -1, 8, 9, 12, 13, 16)), ("min_points", (0, -3))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)
    for dims in ((0, 9, 10), (8, -1, 10), (8, 9, 1025)):
        assert call(dims=dims) == E_VALUE
    for step in ((0.25, 0.25, 0.5), (0.0, 0.0, 0.0), (-0.25,) * 3, (float("nan"),) * 3, (float("inf"),) * 3, (1e-45,) * 3):
        assert call(step=step) == E_VALUE, step
    assert call(origin=(0.0, float("nan"), 0.0)) == E_VALUE
    assert call(dims=(1024, 1024, 512), workspace_words=2 ** 62) == E_VALUE               # 5 * 2^29 cells
    assert call(num_points=0) == E_SHAPE
    assert call(num_points=2 ** 29, workspace_words=2 ** 62) == E_SHAPE                   # 5 * 2^29 points
    assert call(capacity=0) == E_SHAPE and call(capacity=2 ** 29) == E_SHAPE
    assert call(workspace_words=need - 1) == E_SHAPE
    assert call(workspace_words=hip.field_nearest_workspace(5, 720, 5000)) == E_SHAPE     # the nearest workspace is too small
    for key in ("points", "cells", "out_points", "weight", "cell_index", "sums", "count", "outside", "workspace"):
        assert call(**{key: None}) == E_NULL, key
    # the build needs no output, the reduce only `outside`, the compact phase no points and no `outside`
    assert call(phases=1, points=None, out_points=None, outside=None) == E_NULL
    assert call(phases=2, points=None, outside=None) == E_NULL and call(phases=10, outside=None, count=None) == E_NULL
    assert call(phases=4, points=None, outside=None, count=None) == E_NULL
    assert call(phases=6, points=None, sums=None) == E_NULL
    assert call(min_points=2 ** 31 - 1, capacity=1, workspace=None) == E_NULL             # the last permitted values
