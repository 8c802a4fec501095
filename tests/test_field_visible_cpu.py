"""Host-side tests of the z-buffer of posed rows (field_volume.FieldView / visible_rows / ``visible_from``; njf_field_visible;
DESIGN.md section 24): the numpy restatement (tests/field_visible_restatement.py) -- the key order, the independence of the row
order, the clipped footprint written out by hand, the tolerance rule at equality, the rows that are not read --, the signatures,
every argument check, raised before any device work (there is no GPU here), the C ABI's symbol and return codes, and the
condition the GPU test relies on: the numpy registration of the section-22 scene from ALL 878 shell rows converges with the cull
and does not without it.

The bound is section 22's ``CONVERGED = 0.05``, derived there (half a pixel of one-sided displacement over a link of 0.4 at 0.7
rad per unit command).  Measured here: |u - planted| = 3.945e-2 with footprint 1, tolerance 0.01 and reach 0.4 (175 of the 878
rows visible in every round), 7.195e-1 without the cull, 2.969e-1 with footprint 0 (459 rows: the far side shows through)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_commands_restatement as F
import field_joints_restatement as J
import field_nearest_restatement as N
import field_visible_restatement as V
import field_voxels_restatement as S
from test_field_nearest_cpu import _chain_scene, _cpu_arguments
from test_field_normals_gpu import _shell
from test_field_voxels_gpu import ANGLES, CONVERGED, HEIGHT, MAX_JUMP, ROUNDS, SHELL_MODEL, SHELL_SEEN, WIDTH, _camera, _z_buffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 26
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


# ---- the key rule -----------------------------------------------------------------------------------------------------------------------
def test_the_key_order_is_the_float_order_with_ties_to_the_lowest_row():
    rng = np.random.default_rng(24)
    z = np.concatenate([rng.uniform(1e-3, 50.0, 500), np.float64(F32(1.5)) * np.ones(40), [np.finfo(F32).tiny, np.finfo(F32).max,
                        1e-45, 1.0, np.nextafter(F32(1.0), F32(2.0))]]).astype(F32)
    z = z[rng.permutation(z.size)]
    key = V.keys_of(z)
    order = np.argsort(key, kind="stable")
    assert (np.diff(z[order].astype(np.float64)) >= 0).all()                          # the float order
    ties = np.diff(z[order].astype(np.float64)) == 0
    assert ties.sum() >= 39 and (np.diff(order)[ties] > 0).all()                      # equal z: the lowest row first
    assert (key < V.EMPTY).all() and int(key.max() >> np.uint64(32)) == 0x7f7fffff    # a finite z never looks empty
    # one pixel: the winner is the first row of the smallest z
    depth, index, covered = V.rasterise(np.zeros(z.size, np.int64), z, z.size, 1, 1, 0)
    assert covered == 1 and depth[0, 0] == z.min() and index[0, 0] == int(np.flatnonzero(z == z.min())[0])


def _image_case(rng, n, height, width):
    pixel = rng.integers(-1, height * width, n)
    z = rng.uniform(0.5, 3.0, n).astype(F32)
    z[rng.random(n) < 0.3] = F32(1.25)                                              # ties
    return pixel, z


def test_the_depth_image_does_not_depend_on_the_row_order():
    rng = np.random.default_rng(25)
    for n, height, width, f in ((1, 1, 1, 0), (65, 5, 3, 1), (257, 1, 7, 4), (4097, 12, 16, 2)):
        pixel, z = _image_case(rng, n, height, width)
        depth, index, covered = V.rasterise(pixel, z, n, height, width, f)
        perm = rng.permutation(n)
        depth_p, index_p, covered_p = V.rasterise(pixel[perm], z[perm], n, height, width, f)
        assert depth_p.tobytes() == depth.tobytes() and covered_p == covered == int((depth > 0).sum())
        won = index >= 0
        assert (won == (index_p >= 0)).all() and (z[index[won]] == depth[won]).all() and (z[perm][index_p[won]] == depth[won]).all()
        values, times = np.unique(z, return_counts=True)
        untied = won & (times[np.searchsorted(values, depth)] == 1)
        assert (perm[index_p[untied]] == index[untied]).all()                         # the index maps through the permutation
        # a winner of its own pixel is visible, and nothing lies in front of the depth
        seen = V.test_rows(pixel, z, depth, 0.0)
        flat = index.reshape(-1)
        own = np.flatnonzero((flat >= 0) & (pixel[flat.clip(0)] == np.arange(height * width)))
        assert seen[flat[own]].all() and (own.size > 0 or n == 1)
        has = pixel >= 0
        assert (depth.reshape(-1)[pixel[has]] <= z[has]).all()


def test_the_clipped_footprint_on_a_3_by_5_image():
    # rows: 0 at the corner (0, 0) z 2; 1 at the edge (1, 4) z 1; 2 in the middle (1, 2) z 3; 3 without a pixel
    pixel, z = np.int64([0, 1 * 5 + 4, 1 * 5 + 2, -1]), F32([2.0, 1.0, 3.0, 0.5])
    depth, index, covered = V.rasterise(pixel, z, 4, 3, 5, 0)
    assert depth.tolist() == [[2, 0, 0, 0, 0], [0, 0, 3, 0, 1], [0, 0, 0, 0, 0]] and covered == 3
    assert index.tolist() == [[0, -1, -1, -1, -1], [-1, -1, 2, -1, 1], [-1, -1, -1, -1, -1]]
    depth, index, covered = V.rasterise(pixel, z, 4, 3, 5, 1)
    assert depth.tolist() == [[2, 2, 3, 1, 1], [2, 2, 3, 1, 1], [0, 3, 3, 1, 1]] and covered == 14
    assert index.tolist() == [[0, 0, 2, 1, 1], [0, 0, 2, 1, 1], [-1, 2, 2, 1, 1]]
    depth, index, covered = V.rasterise(pixel, z, 4, 3, 5, 2)                        # row 1 (z 1) takes columns 2 .. 4, row 0 the rest
    assert depth.tolist() == [[2, 2, 1, 1, 1]] * 3 and index.tolist() == [[0, 0, 1, 1, 1]] * 3 and covered == 15
    depth, index, covered = V.rasterise(pixel, z, 4, 3, 5, 4)                        # a footprint larger than the image
    assert depth.tolist() == [[1.0] * 5] * 3 and (index == 1).all() and covered == 15
    # a centre just outside the image still reaches in: row 3 at (-1, 5), off the upper right corner, with z 0.5
    depth, index, covered = V.rasterise(pixel, z, 4, 3, 5, 1, outside=[[3, -1, 5]])
    assert depth[0].tolist() == [2, 2, 3, 1, 0.5] and index[0].tolist() == [0, 0, 2, 1, 3] and covered == 14
    assert V.rasterise(pixel, z, 4, 3, 5, 1, outside=[[3, -2, 5]])[0].tobytes() == V.rasterise(pixel, z, 4, 3, 5, 1)[0].tobytes()


def test_the_tolerance_rule_at_equality():
    tol = 0.01
    zmin = F32(2.0)
    edge = zmin + F32(tol) * zmin                       # 2.02 in fp32: z - zmin == tol * zmin?
    at = F32(zmin + (F32(tol) * zmin).astype(F32))
    assert F32(at - zmin) <= F32(F32(tol) * zmin)       # the rule is inclusive where the subtraction lands on the product
    above = np.nextafter(at, F32(10.0))
    z = F32([2.0, at, above, 1.0, np.nan, 2.0])
    pixel = np.int64([0, 0, 0, 0, 0, -1])
    depth = F32([[2.0]])
    want = [True, bool(F32(at - zmin) <= F32(F32(tol) * zmin)), bool(F32(above - zmin) <= F32(F32(tol) * zmin)), True, False, False]
    assert V.test_rows(pixel, z, depth, tol).tolist() == want and want[1] and not want[2]
    assert V.test_rows(pixel, z, depth, 0.0).tolist() == [True, False, False, True, False, False]   # tolerance 0: the winner and its ties
    assert float(edge) > 2.0


def test_rows_that_are_not_read_are_not_splatted_and_get_the_fill_values():
    k = np.array([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]])
    c2w = np.eye(4)[None]
    pts = F32([[0, 0, 1.0], [0, 0, 0.5], [np.nan, 0, 0.4], [0, np.inf, 0.3], [0, 0, 0.2], [0, 0, 0.1], [0, 0, -1.0], [0, 0, 0.0]])
    labels = np.int32([0, 3, 0, 0, -1, 0, 0, 0])
    out = V.visible(pts, k, c2w, 3, 3, footprint=0, tolerance=0.0, count=5, labels=labels)
    # row 1 (z 0.5) wins the centre pixel: rows 2, 3 are not finite, row 4 has a negative label, rows 5.. lie from the count on
    assert out["depth"][0, 0].tolist() == [[0, 0, 0], [0, 0.5, 0], [0, 0, 0]] and out["index"][0, 0, 1, 1] == 1
    assert out["seen"].tolist() == [[0, 1, 0, 0, 0, 0, 0, 0]] and out["visible"].tolist() == [1] and out["covered"].tolist() == [[1]]
    assert out["pixel"][0, 0].tolist() == [4, 4, -1, -1, -1, -1, -1, -1]
    assert np.isnan(out["z"][0, 0, 2:]).all() and out["z"][0, 0, :2].tolist() == [1.0, 0.5]
    assert np.isnan(out["culled"][0, [0, 2, 3, 4, 5, 6, 7]]).all() and out["culled"][0, 1].tobytes() == pts[1].tobytes()
    # read, but behind the camera or at z == near: a z, no pixel, not seen
    out = V.visible(pts, k, c2w, 3, 3, footprint=0, tolerance=0.0, near=0.1)
    assert out["pixel"][0, 0].tolist() == [4, 4, -1, -1, 4, -1, -1, -1] and out["z"][0, 0, 5:].tolist() == [F32(0.1), -1.0, 0.0]
    assert out["seen"].tolist() == [[0, 0, 0, 0, 1, 0, 0, 0]]
    # tolerance: everything within 150 % of the nearest
    assert V.visible(pts, k, c2w, 3, 3, footprint=0, tolerance=1.5, near=0.1)["seen"].tolist() == [[0, 1, 0, 0, 1, 0, 0, 0]]
    # two views: the second camera looks back along -z (a rotation about y) and sees rows 6 only; Mq = 1 for two problems
    back = np.diag([-1.0, 1.0, -1.0, 1.0])
    out = V.visible(pts, np.concatenate([k, k]), np.stack([c2w[0], back]), 3, 3, footprint=0, tolerance=0.0, problems=2)
    assert out["seen"].tolist() == [[0, 0, 0, 0, 0, 1, 2, 0]] * 2 and out["visible"].tolist() == [2, 2]


def test_the_projection_is_the_pixel_grid_of_depth_points():
    """A point back-projected from a pixel centre (field_voxels_restatement.pinhole_points) projects into that pixel, at that z."""
    rng = np.random.default_rng(26)
    k, c2w = _camera()
    depth = rng.uniform(0.5, 3.0, (1, HEIGHT, WIDTH)).astype(F32)
    pts = S.pinhole_points(depth, k, c2w, "z")[0]
    pr = V.project(pts, k, c2w, HEIGHT, WIDTH)
    assert (pr["pixel"][0, 0] == np.arange(HEIGHT * WIDTH)).all() and np.abs(pr["z"][0, 0] - depth.reshape(-1)).max() < 1e-6
    assert np.abs(pr["x"][0, 0] - np.floor(pr["x"][0, 0]) - 0.5).max() < 1e-4


# ---- the interface ------------------------------------------------------------------------------------------------------------------------
def test_the_signatures():
    from neural_jacobian_field_amd import field_volume as fv
    from neural_jacobian_field_amd import hip
    params = inspect.signature(fv.visible_rows).parameters
    assert list(params) == ["points", "view", "labels", "count"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None for k in ("labels", "count"))
    fields = fv.FieldView.__dataclass_fields__
    assert list(fields) == ["intrinsics", "cam2world", "height", "width", "footprint", "tolerance", "near"]
    assert (fields["footprint"].default, fields["tolerance"].default, fields["near"].default) == (1, 0.01, 0.0)
    assert list(fv.FieldVisibility.__dataclass_fields__) == ["seen", "culled", "visible", "depth", "index", "covered", "pixel", "z"]
    assert [name for name, _ in hip.FIELD_VISIBLE_OUTPUTS] == ["depth", "index", "covered", "seen", "culled", "visible", "pixel", "z"]
    # the registrations with the cull: register_commands' arguments with the view behind them, the information as a keyword
    for fn, plain in ((fv.register_commands_visible, fv.register_commands), (fv.cloud_registration_visible, fv.cloud_registration)):
        params, base = inspect.signature(fn).parameters, inspect.signature(plain).parameters
        positional = [k for k, v in base.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
        keywords = {k: v.default for k, v in base.items() if v.kind is v.KEYWORD_ONLY}
        assert list(params) == positional + ["visible_from", "observed_information"] + list(keywords)
        assert params["visible_from"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and params["visible_from"].default is inspect.Parameter.empty
        assert params["observed_information"].kind is inspect.Parameter.KEYWORD_ONLY and params["observed_information"].default is None
        assert {k: params[k].default for k in keywords} == keywords and all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    assert issubclass(fv.FieldVisibleRegistration, fv.FieldRegistration)
    assert list(fv.FieldVisibleRegistration.__dataclass_fields__) == list(fv.FieldRegistration.__dataclass_fields__) + ["visible_history"]
    assert "depth_points(kind=\"z\")" in fv.FieldVisibility.__doc__ and "depth_points(kind=\"z\")" in fv.visible_rows.__doc__
    assert list(inspect.signature(hip.field_visible_workspace).parameters) == ["m", "v", "h", "w"]


def _view(**kw):
    from neural_jacobian_field_amd.field_volume import FieldView
    k, c2w = _camera()
    args = dict(intrinsics=torch.from_numpy(k), cam2world=torch.from_numpy(c2w), height=48, width=64)
    args.update(kw)
    return FieldView(**args)


def _bad_views():
    """(pattern, view) for every way a FieldView can be wrong."""
    k, c2w = (torch.from_numpy(v) for v in _camera())
    bad = [("intrinsics must be fp32 \\[V, 3, 3\\] with 1 <= V <= 32", _view(intrinsics=v))
           for v in (None, k.double(), k[0], k[:, :2], k.expand(33, 3, 3), k[:0], k.numpy())]
    bad += [("cam2world must be fp32 \\[1, 4, 4\\]", _view(cam2world=v)) for v in (None, c2w.double(), c2w[0], c2w.expand(2, 4, 4), c2w[:, :3])]
    bad += [("height must be an integer >= 1", _view(height=v)) for v in (0, -1, 48.0, True, None)]
    bad += [("width must be an integer >= 1", _view(width=v)) for v in (0, 64.0, False, "64")]
    bad += [("footprint must be an integer in \\[0, 4\\]", _view(footprint=v)) for v in (-1, 5, 1.0, True, None)]
    bad += [("near must be a finite number >= 0", _view(near=v)) for v in (-0.1, float("nan"), float("inf"), 1e39, None, True, "0")]
    bad += [("tolerance must be a finite number >= 0", _view(tolerance=v)) for v in (-1e-3, float("nan"), float("inf"), None, False)]
    bad += [("M \\* V \\* height \\* width must stay below 2\\*\\*31", _view(height=2 ** 15, width=2 ** 15))]
    return bad


def test_visible_rows_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import visible_rows
    pts = torch.zeros(2, 40, 3)
    for bad in (None, pts.double(), pts[..., :2], pts[0, 0], np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="visible_rows: points must be fp32 \\[n, 3\\] or \\[M, n, 3\\]"):
            visible_rows(bad, _view())
    for bad in (torch.zeros(0, 40, 3), torch.zeros(65536, 1, 3)):
        with pytest.raises(ValueError, match="visible_rows: 1 to 65535 problems"):
            visible_rows(bad, _view())
    for bad in (None, _camera(), dict(height=48)):
        with pytest.raises(ValueError, match="visible_rows: the view must be a FieldView"):
            visible_rows(pts, bad)
    for pattern, view in _bad_views():
        with pytest.raises(ValueError, match="visible_rows: " + pattern):
            visible_rows(pts, view)
    with pytest.raises(ValueError, match="visible_rows: M \\* V \\* n must stay below 2\\*\\*31"):
        visible_rows(torch.zeros(1, 3).expand(2 ** 15, 2 ** 16, 3), _view(height=1, width=1))
    for bad in (3, torch.ones(2, dtype=torch.int32), torch.ones(1)):
        with pytest.raises(ValueError, match="visible_rows: count must be one int32"):
            visible_rows(pts, _view(), count=bad)
    for bad in (torch.zeros(40), torch.zeros(39, dtype=torch.int32), [0] * 40):
        with pytest.raises(ValueError, match="visible_rows: labels must be int32 \\[40\\]"):
            visible_rows(pts, _view(), labels=bad)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="visible_rows: intrinsics must live on the device of points"):
            visible_rows(pts.cuda(), _view())
        with pytest.raises(ValueError, match="visible_rows: labels must live on the device of points"):
            view = _view()
            view.intrinsics, view.cam2world = view.intrinsics.cuda(), view.cam2world.cuda()
            visible_rows(pts.cuda(), view, labels=torch.zeros(40, dtype=torch.int32))
    for args, kw in (((pts, _view()), {}), ((pts[0], _view(footprint=0, tolerance=0.0, near=0.5)), {}),
                     ((pts, _view(footprint=4)), dict(count=torch.ones(1, dtype=torch.int32), labels=torch.zeros(40, dtype=torch.int32)))):
        with pytest.raises(ValueError, match="visible_rows: .*no CPU path"):
            visible_rows(*args, **kw)


def test_the_registrations_with_the_cull_check_their_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud, cell_grid, cloud_registration_visible, register_commands_visible
    tw, joints, tree, xyz, labels, obs = _cpu_arguments()
    chain = J.chain()
    n = xyz.shape[0]
    cells = cell_grid((0, 0, 0), (1, 1, 1), 0.1)
    info = torch.zeros(2, 50, 6)
    cloud = FieldPointCloud(grid=FieldGrid(chain["origin"], chain["step"], chain["dims"]), index=torch.from_numpy(chain["index"]),
                            xyz=xyz, density=torch.ones(n), color=None, jacobian=None, count=torch.tensor([n], dtype=torch.int32))
    calls = (("register_commands_visible", lambda visible_from, **kw: register_commands_visible(tw, xyz, labels, obs, cells, 0.1, visible_from, **kw)),
             ("register_commands_visible", lambda visible_from, **kw: register_commands_visible(tw, xyz, labels, obs, cells, 0.1, visible_from,
                                                                                                observed_information=info, **kw)),
             ("cloud_registration_visible", lambda visible_from, **kw: cloud_registration_visible(cloud, labels, tw, obs, 0.1, visible_from, **kw)),
             ("cloud_registration_visible", lambda visible_from, **kw: cloud_registration_visible(cloud, labels, tw, obs, 0.1, visible_from,
                                                                                                  observed_information=info, **kw)))
    for name, go in calls:
        for bad in (_camera(), 1, "view", None):
            with pytest.raises(ValueError, match=name + ": the view must be a FieldView"):
                go(visible_from=bad)
        for pattern, view in _bad_views():
            with pytest.raises(ValueError, match=name + ": " + pattern):
                go(visible_from=view)
        with pytest.raises(ValueError, match=name + ": reg must be"):          # register_commands' own checks, under this name
            go(visible_from=_view(), reg=-1.0)
        with pytest.raises(ValueError, match=name + ": rounds must be an integer"):
            go(visible_from=_view(), rounds=0)
        for view in (_view(), _view(footprint=0, tolerance=0.5, near=0.25)):
            with pytest.raises(ValueError, match=name + ": .*no CPU path"):
                go(visible_from=view)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="register_commands_visible: intrinsics must live on the device of xyz"):
            register_commands_visible(tw, xyz.cuda(), labels.cuda(), obs.cuda(), cells, 0.1, _view())
    with pytest.raises(ValueError, match="register_commands_visible: observed_information must be fp32"):
        register_commands_visible(tw, xyz, labels, obs, cells, 0.1, _view(), observed_information=info[..., :5])
    with pytest.raises(ValueError, match="cloud_registration_visible: cloud must be a FieldPointCloud"):
        cloud_registration_visible(None, labels, tw, obs, 0.1, _view())


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    assert "njf_field_visible" in declared and "njf_field_visible" in hip.EXPORTED_SYMBOLS and hasattr(lib, "njf_field_visible")
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    params = re.search(r"njf_field_visible\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_visible.argtypes) == ARGUMENTS
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_VISIBLE_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_VISIBLE_ALL"] == hip.FIELD_VISIBLE_ALL == sum(hip.FIELD_VISIBLE_PHASES) == 7
    assert [defines[f"NJF_FIELD_VISIBLE_{n.upper()}"] for n in hip.FIELD_VISIBLE_PHASE_NAMES] == list(hip.FIELD_VISIBLE_PHASES)
    assert defines["NJF_FIELD_VISIBLE_DIRECT"] == hip.FIELD_VISIBLE_DIRECT == 8
    assert defines["NJF_FIELD_VISIBLE_MAX_VIEWS"] == hip.FIELD_VISIBLE_MAX_VIEWS == V.MAX_VIEWS == 32
    assert defines["NJF_FIELD_VISIBLE_MAX_FOOTPRINT"] == hip.FIELD_VISIBLE_MAX_FOOTPRINT == V.MAX_FOOTPRINT == 4
    assert "#define NJF_FIELD_VISIBLE_WORKSPACE(M, V, H, W) (2LL * (M) * (V) * (H) * (W) + 1LL)" in header
    assert hip.field_visible_workspace(3, 2, 48, 64) == 2 * 3 * 2 * 48 * 64 + 1


def test_the_default_form_of_the_splat_follows_the_environment(monkeypatch):
    from neural_jacobian_field_amd import hip
    monkeypatch.delenv("NJF_FIELD_VISIBLE_DIRECT", raising=False)
    assert hip.field_visible_default_phase() == hip.FIELD_VISIBLE_ALL
    monkeypatch.setenv("NJF_FIELD_VISIBLE_DIRECT", "1")
    assert hip.field_visible_default_phase() == hip.FIELD_VISIBLE_ALL | hip.FIELD_VISIBLE_DIRECT
    monkeypatch.setenv("NJF_FIELD_VISIBLE_DIRECT", "0")
    assert hip.field_visible_default_phase() == hip.FIELD_VISIBLE_ALL


def test_the_entry_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("points", "count", "labels", "num_queries", "n", "num_problems", "k", "w2c", "views", "height", "width", "footprint", "near",
             "tolerance", "depth", "index", "covered", "seen", "culled", "visible", "pixel", "z", "workspace", "workspace_words", "phases")
    need = hip.field_visible_workspace(3, 2, 48, 64)

    def call(**kw):
        args = {k: P for k in names}
        args.update(num_queries=3, n=500, num_problems=3, views=2, height=48, width=64, footprint=1, near=0.0, tolerance=0.01,
                    workspace_words=need, phases=7)
        args.update(kw)
        return lib.njf_field_visible(*[args[k] for k in names], None)

    # every call that could pass its checks is given a workspace that is too small, so that none reaches a launch
    assert call(workspace_words=need - 1) == E_SHAPE
    for key in ("points", "k", "w2c", "depth", "index", "covered", "seen", "culled", "visible", "pixel", "z", "workspace"):
        assert call(**{key: None}) == E_NULL, key
    assert call(count=None, labels=None, workspace_words=0) == E_SHAPE                 # the two optional inputs
    # what a phase does not touch may be missing
    assert call(phases=1, workspace_words=0, depth=None, index=None, covered=None, seen=None, culled=None, visible=None, pixel=None,
                z=None) == E_SHAPE
    assert call(phases=9, workspace_words=0, depth=None) == E_SHAPE
    assert call(phases=2, workspace_words=0, points=None, seen=None, culled=None, visible=None, pixel=None, z=None) == E_SHAPE
    assert call(phases=2, index=None) == E_NULL and call(phases=1, points=None) == E_NULL and call(phases=3, workspace=None) == E_NULL
    assert call(phases=4, n=-1, workspace=None, index=None, covered=None) == E_SHAPE   # the test reads no workspace
    assert call(phases=4, depth=None) == E_NULL and call(phases=4, z=None) == E_NULL and call(phases=6, covered=None) == E_NULL
    for key, values in (("phases", (0, -1, 8, 10, 12, 14, 16, 23)), ("num_problems", (0, -1, 65536)), ("num_queries", (0, 2, 4, -3)),
                        ("views", (0, -1, 33)), ("footprint", (-1, 5, 100)),
                        ("near", (-1.0, float("nan"), float("inf"))), ("tolerance", (-1e-3, float("nan"), float("inf")))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)
            assert call(**{key: bad}, n=-1) == E_VALUE, (key, bad)                     # (judged before the shapes)
    assert call(num_queries=1, workspace_words=0) == E_SHAPE                           # Mq = 1 is fine
    for kw in (dict(n=-1), dict(height=0), dict(width=0), dict(height=-4), dict(height=2 ** 16, width=2 ** 15),
               dict(height=2 ** 14, width=2 ** 14, num_problems=4, num_queries=4), dict(n=2 ** 29, num_problems=2, num_queries=2),
               dict(n=2 ** 30, num_problems=1, num_queries=1)):
        assert call(**kw, workspace_words=2 ** 62) == E_SHAPE, kw
    assert call(workspace_words=hip.field_visible_workspace(3, 2, 48, 63)) == E_SHAPE


# ---- the condition of the GPU test, on the CPU --------------------------------------------------------------------------------------------
def section_22_scene(angles=ANGLES):
    """The scene of test_field_voxels_gpu's end-to-end test without a device: the chain with ALL rows of its shell at
    ``SHELL_MODEL`` subdivisions (878), the camera, the 48 x 64 depth image of the shell at ``SHELL_SEEN`` posed at the planted
    command, and the cloud of its back-projection (float64 pinhole model, rounded) under max_jump, NaN where a pixel gives none."""
    s = _chain_scene()
    k, c2w = _camera()
    s["xyz"], s["labels"] = _shell(s["scene"], SHELL_MODEL)
    fine_xyz, fine_labels = _shell(s["scene"], SHELL_SEEN)
    planted = np.float32([[angles[0] / 0.7, angles[1] / 1.3, 0.0]])
    posed = F.posed_targets(s["twists"], planted, fine_xyz, fine_labels, s["parts"], s["joints"], s["tree"])[0]
    depth = _z_buffer(posed, k[0], c2w[0], HEIGHT, WIDTH)[None]
    observed = S.pinhole_points(depth, k, c2w, "z")[0].astype(np.float32)
    observed[~S.depth_mask(depth, max_jump=MAX_JUMP).reshape(-1)] = np.nan
    return s, k, c2w, planted, depth, observed


def restated_registration(s, k, c2w, observed, footprint=1, tolerance=0.01, cull=True, height=HEIGHT, width=WIDTH):
    history = []
    search = V.cull(k, c2w, height, width, footprint, tolerance, history=history) if cull else N.brute
    out = N.register(s["twists"], s["xyz"], s["labels"], observed, 4 * s["step"], s["parts"], s["joints"], s["tree"], rounds=ROUNDS,
                     iterations=3, search=search)
    out["visible_history"] = np.stack(history).astype(np.int32) if history else None
    return out


def test_the_cull_makes_the_whole_shell_register_to_a_depth_image():
    s, k, c2w, planted, depth, observed = section_22_scene()
    assert s["xyz"].shape[0] == 878 and abs(4 * s["step"] - 0.4) < 1e-12
    culled = restated_registration(s, k, c2w, observed)
    plain = restated_registration(s, k, c2w, observed, cull=False)
    gaps = restated_registration(s, k, c2w, observed, footprint=0)
    d_culled, d_plain, d_gaps = (float(np.abs(r["fit"]["commands"] - planted).max()) for r in (culled, plain, gaps))
    print(f"|u - planted|: culled {d_culled:.3e} (visible {culled['visible_history'][:, 0].tolist()}), no cull {d_plain:.3e}, "
          f"footprint 0 {d_gaps:.3e} (visible {gaps['visible_history'][:, 0].tolist()})")
    assert d_culled <= CONVERGED                          # the condition the GPU test relies on
    assert d_plain > 4 * CONVERGED                        # rows of the far side are matched to the near side
    assert d_gaps > 4 * CONVERGED                         # the far side shows through the gaps: the footprint is part of the feature
    assert abs(d_culled - 3.945e-2) < 5e-5 and (culled["visible_history"] == 175).all()      # the figures of the issue
    assert culled["found_history"].tolist() == culled["visible_history"].tolist()           # every visible row finds a point within reach
    # the depth image the cull renders of the rows at the planted command is a depth image of the same body: it covers the
    # pixels of the observation's front faces
    seen = V.visible(F.posed_targets(s["twists"], planted, s["xyz"], s["labels"], s["parts"], s["joints"], s["tree"]), k, c2w, HEIGHT,
                     WIDTH, 1, 0.01)
    both = (seen["depth"][0, 0] > 0) & (depth[0] > 0)
    assert both.sum() > 500 and np.abs(seen["depth"][0, 0][both] - depth[0][both]).max() < 0.5
