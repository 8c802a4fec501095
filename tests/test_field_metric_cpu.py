"""Host-side tests of inverse kinematics with a 3 x 3 information per target (field_volume.solve_commands_metric and its
companions; njf_field_commands_metric): the numpy restatement (tests/field_metric_restatement.py) -- the
74-moment form against sums over the rows, planted commands from the pixel rays of one camera and from planes, the identity
information against section 18, the rows left out --, the helpers against numpy, the signatures, every argument check raised
before any device work, and the C ABI's symbol and return codes.  There is no GPU here.

``E_m = sum w tr(Q) (|x~|^2 + |y~|^2)`` over the counted rows is the scale of the moment form's cancellation."""
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_commands_restatement as F
import field_joints_restatement as J
import field_metric_restatement as M
import field_pose_restatement as R
from neural_jacobian_field_amd.field_volume import FieldMetricCommands, solve_commands_metric  # noqa: F401  (what is under test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 47
K_NORM = np.float64([[1.2, 0.0, 0.5], [0.0, 1.2, 0.5], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


@pytest.fixture(scope="module")
def chain():
    scene = J.chain()
    ref = J.run(scene)
    tree = (np.array([-1, 0, 1], np.int32), np.array([-1, 0, 1], np.int32))
    xyz = J.node_coordinates(scene["dims"], scene["index"]).astype(np.float32)
    return dict(scene=scene, twists=R.twists_of(scene), joints=R.joints_of(ref), tree=tree, xyz=xyz, labels=scene["labels"],
                parts=scene["parts"])


@pytest.fixture(scope="module")
def face():
    scene = J.face()
    scene["omega"], scene["velocity"] = 0.3 * scene["omega"], 0.05 * scene["velocity"]
    xyz = J.node_coordinates(scene["dims"], scene["index"]).astype(np.float32)
    return dict(scene=scene, twists=R.twists_of(scene), joints=None, tree=None, xyz=xyz, labels=scene["labels"], parts=scene["parts"])


def _targets(s, commands, **kw):
    return F.posed_targets(s["twists"], np.asarray(commands, np.float32), s["xyz"], s["labels"], s["parts"], s["joints"], s["tree"], **kw)


def _solve(s, targets, information, **kw):
    return M.solve(s["twists"], s["xyz"], s["labels"], targets, information, s["parts"], s["joints"], s["tree"], **kw)


def _energy(s, targets, information, weights=None):
    status, _ = F.pose_status(s["twists"], s["joints"], s["tree"])
    return M.energy(s["xyz"], s["labels"], targets, information, s["parts"], s["twists"]["count"], status, s["twists"]["centroid"], weights)


def _random_psd(rng, shape):
    a = rng.normal(size=shape + (3, 3))
    return M.pack(a @ np.swapaxes(a, -1, -2))


def _extent(s):
    rows = s["labels"] >= 0
    return float(np.linalg.norm(s["xyz"][rows].max(axis=0) - s["xyz"][rows].min(axis=0)))


def _camera(s, side, extents):
    """(intrinsics [1, 3, 3], cam2world [1, 4, 4]) of a camera ``extents`` body extents from the body's centre along ``side``."""
    rows = s["labels"] >= 0
    centre = 0.5 * (s["xyz"][rows].max(axis=0) + s["xyz"][rows].min(axis=0)).astype(np.float64)
    eye = centre + extents * _extent(s) * np.asarray(side, dtype=np.float64) / np.linalg.norm(side)
    # the focal length grows with the distance, so that the body fills the same part of the frame
    k = K_NORM.copy()
    k[0, 0] = k[1, 1] = 0.4 * extents
    return k[None].astype(np.float32), M.look_at(eye, centre)[None].astype(np.float32)


# ---- the moment form ----------------------------------------------------------------------------------------------------------------
def test_the_moment_form_is_the_sum_over_the_rows(chain, face):
    worst = 0.0
    for s, u, at in ((chain, [[0.9, -0.5, 0.3], [0.2, 0.7, 0.0]], [0.3, 0.2, -0.4]),
                     (face, 0.3 * np.random.default_rng(1).uniform(-1, 1, (2, 10)), np.linspace(-0.2, 0.2, 10))):
        targets = _targets(s, u)
        rng = np.random.default_rng(2)
        weights = rng.uniform(0.1, 2.0, size=targets.shape[:2]).astype(np.float32)
        information = _random_psd(rng, targets.shape[:2])
        status, _ = F.pose_status(s["twists"], s["joints"], s["tree"])
        mom, _ = M.moments(s["xyz"], s["labels"], targets, information, s["parts"], None, status, s["twists"]["centroid"], weights)
        slot, w = M.counted(s["xyz"], s["labels"], targets, information, s["parts"], None, status, weights)
        energy, total = _energy(s, targets, information, weights)
        pose = F.chain(s["twists"], np.float32(at), s["joints"], s["tree"])
        for m in range(targets.shape[0]):
            c0, g0, h0, w0 = M.evaluate_moments(mom[m], pose, s["twists"]["centroid"])
            c1, g1, h1, w1 = M.evaluate_rows(s["xyz"], slot, w[m], targets[m], information[m], pose)
            ratio = abs(c0 - c1) / (1e-13 * energy[m] / total[m])
            worst = max(worst, ratio)
            print("moment form: cost / bound", ratio, "g", np.abs(g0 - g1).max() / np.abs(g1).max(), "H", np.abs(h0 - h1).max() / np.abs(h1).max())
            assert abs(w0 - w1) <= 1e-12 * w1 and abs(w0 - total[m]) <= 1e-12 * w1
            assert ratio <= 1.0
            assert np.abs(g0 - g1).max() <= 1e-12 * np.abs(g1).max() and np.abs(h0 - h1).max() <= 1e-12 * np.abs(h1).max()
            assert np.abs(h0 - h0.T).max() <= 1e-15 * np.abs(h0).max()
    assert worst > 0.0


# ---- planted commands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extents", (4.0, 40.0))
def test_one_camera_recovers_planted_commands_from_its_pixel_rays(chain, extents):
    planted = np.float32([[0.6, -0.4, 0.0]])
    moved = _targets(chain, planted)
    for side in ((1.0, 0.2, 0.3), (0.2, 1.0, -0.3), (0.3, -0.2, 1.0)):
        k, c2w = _camera(chain, side, extents)
        pixels = M.project(moved, k, c2w).astype(np.float32)
        assert np.isfinite(pixels).all() and pixels.min() > 0.0 and pixels.max() < 1.0        # every row is in the frame
        targets, information = M.ray_targets(chain["xyz"], pixels, k, c2w)
        out = _solve(chain, targets, information)
        print(f"camera on {side} at {extents} extents: steps {out['steps']}, commands {out['commands']}, cost {out['cost']}")
        assert not out["status"].any()
        assert np.abs(out["commands"] - planted).max() <= 1e-5


def _slid(s, moved, rng, amount):
    """(targets, information): every moved row slid by ``amount`` inside a plane of a random unit normal through it."""
    normals = rng.normal(size=moved.shape)
    normals /= np.linalg.norm(normals, axis=-1, keepdims=True)
    slide = np.cross(normals, rng.normal(size=moved.shape))
    slide *= amount / np.linalg.norm(slide, axis=-1, keepdims=True)
    normals = normals.astype(np.float32)
    # (the slide is orthogonal to the fp32 normal the solver sees, up to the rounding of the fp32 target)
    n64 = normals.astype(np.float64)
    slide -= n64 * (slide * n64).sum(axis=-1, keepdims=True) / (n64 * n64).sum(axis=-1, keepdims=True)
    return (moved.astype(np.float64) + slide).astype(np.float32), M.plane_information(normals)


def test_planes_recover_planted_commands_where_points_do_not(chain):
    planted = np.float32([[0.6, -0.4, 0.0]])
    moved = _targets(chain, planted)
    targets, information = _slid(chain, moved, np.random.default_rng(3), 0.5 * _extent(chain))
    plane = _solve(chain, targets, information)
    point = F.solve(chain["twists"], chain["xyz"], chain["labels"], targets, chain["parts"], chain["joints"], chain["tree"])
    print("planes:", plane["commands"], "points:", point["commands"])
    assert not plane["status"].any() and np.abs(plane["commands"] - planted).max() <= 1e-5
    assert np.abs(point["commands"] - planted).max() > 1e-2


def test_the_identity_information_is_section_18(chain, face):
    for s, u in ((chain, [[0.5, 0.3, 0.0], [-0.8, 0.6, 0.0]]), (face, 0.2 * np.random.default_rng(6).uniform(-1, 1, (2, 10)))):
        rng = np.random.default_rng(7)
        targets = (_targets(s, u) + 0.02 * rng.normal(size=(2, s["xyz"].shape[0], 3))).astype(np.float32)
        weights = rng.uniform(0.2, 2.0, s["xyz"].shape[0]).astype(np.float32)
        identity = np.broadcast_to(M.IDENTITY6, (s["xyz"].shape[0], 6))
        ours = _solve(s, targets, identity, weights=weights)
        theirs = F.solve(s["twists"], s["xyz"], s["labels"], targets, s["parts"], s["joints"], s["tree"], weights=weights)
        energy, total = _energy(s, targets, identity, weights)
        e18, w18 = F.energy(theirs["moments"])
        assert np.allclose(energy, 3.0 * e18, rtol=1e-12) and np.allclose(total, w18, rtol=1e-12)       # tr(I) = 3
        assert np.abs(ours["commands"] - theirs["commands"]).max() <= 1e-6
        assert (np.abs(ours["cost"] - theirs["cost"]) <= 1e-13 * energy / total).all()
        assert (np.abs(ours["initial_cost"] - theirs["initial_cost"]) <= 1e-13 * energy / total).all()
        assert ours["status"].tolist() == theirs["status"].tolist() and np.array_equal(ours["weight"], theirs["weight"])


def test_rows_are_left_out_and_bounds_and_the_regulariser_hold(chain):
    planted = np.float32([[0.6, -0.4, 0.0]] * 3)
    moved = _targets(chain, planted)
    rng = np.random.default_rng(8)
    targets, information = _slid(chain, moved, rng, 0.1)
    information = information.copy()
    tip = np.flatnonzero(chain["labels"] == chain["parts"][2])
    body = np.flatnonzero(chain["labels"] >= 0)
    bad_q, bad_y = rng.choice(body, 30, replace=False), rng.choice(body, 30, replace=False)
    for e, row in enumerate(bad_q):
        information[0, row, e % 6] = np.nan if e % 2 else np.inf
    targets[0, bad_y, 1] = np.nan
    information[1] = np.nan
    information[1, tip[[0, 5, 40, 63]]] = M.IDENTITY6                    # four handles with a full 3-D target
    targets[1, tip[[0, 5, 40, 63]]] = moved[1, tip[[0, 5, 40, 63]]]
    targets[2] = np.nan
    out = _solve(chain, targets, information, init=np.float32([[0, 0, 0], [0, 0, 0], [0.2, -3.0, 1.0]]), lower=-1.0, upper=1.0)
    left = len(set(bad_q.tolist()) | set(bad_y.tolist()))
    assert out["weight"].tolist() == [float(len(body) - left), 4.0, 0.0] and out["status"].tolist() == [0, 0, F.NO_ROWS]
    assert out["commands"][2].tolist() == [np.float32(0.2), -1.0, 1.0] and not out["moments"][2].any() and out["cost"][2] == 0.0
    assert np.abs(out["commands"][:2] - planted[:2]).max() <= 1e-5
    # the same problem without the rows equals the problem with them left out
    keep = np.ones(chain["xyz"].shape[0], bool)
    keep[list(set(bad_q.tolist()) | set(bad_y.tolist()))] = False
    again = _solve(chain, np.where(keep[None, :, None], targets[:1], np.float32(np.nan)),
                   np.where(keep[None, :, None], information[:1], np.float32(0.0)))
    assert np.array_equal(again["moments"][0], out["moments"][0])
    # the box and the regulariser
    clean_t, clean_q = _slid(chain, _targets(chain, [[0.9, -0.7, 0.0]]), rng, 0.1)
    boxed = _solve(chain, clean_t, clean_q, lower=-0.5, upper=0.5)
    assert boxed["commands"].tolist() == [[0.5, -0.5, 0.0]]
    assert boxed["gradient"][0, 0] < 0.0 and boxed["gradient"][0, 1] > 0.0 and boxed["gradient"][0, 2] == 0.0
    free, held = _solve(chain, clean_t, clean_q), _solve(chain, clean_t, clean_q, reg=1e-3)
    assert np.linalg.norm(held["commands"]) < np.linalg.norm(free["commands"]) and held["cost"][0] > free["cost"][0]
    assert np.abs(held["gradient"]).max() <= 1e-7
    with np.errstate(invalid="ignore"):
        not_finite = _solve(chain, clean_t, clean_q, init=np.float32([[np.inf, 0.0, 0.0]]))
    assert not_finite["status"].tolist() == [F.NOT_FINITE] and not_finite["steps"].tolist() == [0]


# ---- the helpers --------------------------------------------------------------------------------------------------------------------
def _torch_rays(coordinates_xy, intrinsics, cam2world):
    o, d = M.world_rays(coordinates_xy.numpy(), intrinsics.numpy(), cam2world.numpy())
    return torch.from_numpy(np.ascontiguousarray(o)).float(), torch.from_numpy(d).float()


def test_the_helpers_against_numpy(chain, monkeypatch):
    from neural_jacobian_field_amd import field_volume, geometry
    rng = np.random.default_rng(9)
    v = rng.normal(size=(2, 7, 3))
    v = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    got = field_volume.plane_information(torch.from_numpy(v))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 7, 6)
    assert np.abs(got.numpy() - M.plane_information(v)).max() <= 2.0 ** -23
    for along in (0.0, 0.04, 1.0):
        got = field_volume.ray_information(torch.from_numpy(v), along)
        assert got.dtype == torch.float32 and np.abs(got.numpy() - M.ray_information(v, along)).max() <= 2.0 ** -22
    assert np.abs(field_volume.ray_information(torch.from_numpy(v), 1.0).numpy() - M.IDENTITY6).max() == 0.0
    q = M.symmetric(field_volume.ray_information(torch.from_numpy(v[0])).numpy())
    along_d = np.einsum("nij,nj->ni", q, v[0].astype(np.float64))                            # Q d = floor d: the depth is all but free
    assert np.abs(along_d).max() <= 1e-6 and (np.einsum("ni,ni->n", along_d, v[0].astype(np.float64)) > 0.0).all()
    assert field_volume.INFORMATION_FLOOR == M.INFORMATION_FLOOR == 2.0 ** -21
    assert torch.equal(field_volume.ray_information(torch.from_numpy(v), 1e-9), field_volume.ray_information(torch.from_numpy(v)))
    for bad in (v, torch.from_numpy(v).double(), torch.zeros(4, 2)):
        with pytest.raises(ValueError, match="plane_information: normals must be fp32"):
            field_volume.plane_information(bad)
        with pytest.raises(ValueError, match="ray_information: directions must be fp32"):
            field_volume.ray_information(bad)
    for bad in (-0.1, 1.5, float("nan"), "0", True):
        with pytest.raises(ValueError, match="ray_information: along must be a number in"):
            field_volume.ray_information(torch.from_numpy(v), bad)
    # ray_targets: the rays are the package's (here their restatement: the launch needs a GPU), the rest is torch
    monkeypatch.setattr(geometry, "get_world_rays", _torch_rays)
    xyz = chain["xyz"]
    n = xyz.shape[0]
    k0, c0 = _camera(chain, (1.0, 0.2, 0.3), 4.0)
    k1, c1 = _camera(chain, (0.3, -0.2, 1.0), 40.0)
    k, c2w = np.concatenate([k0, k1]), np.concatenate([c0, c1])
    pixels = M.project(_targets(chain, [[0.6, -0.4, 0.0]] * 2), k, c2w).astype(np.float32)
    pixels[0, 5, 0] = np.nan
    pixels[1, 9] = np.inf
    targets, information = field_volume.ray_targets(*(torch.from_numpy(t) for t in (xyz, pixels, k, c2w)))
    want_t, want_q = M.ray_targets(xyz, pixels, k, c2w)
    assert targets.dtype == information.dtype == torch.float32 and tuple(targets.shape) == (2, n, 3) and tuple(information.shape) == (2, n, 6)
    free = np.isnan(want_t).all(axis=-1)
    assert free.sum() == 2 and free[0, 5] and free[1, 9] and np.array_equal(np.isnan(targets.numpy()).all(axis=-1), free)
    scale = np.abs(c2w[:, :3, 3]).max()
    assert np.abs(targets.numpy()[~free] - want_t[~free]).max() <= 8 * 2.0 ** -23 * scale
    assert np.abs(information.numpy()[~free] - want_q[~free]).max() <= 4 * 2.0 ** -23
    # the foot lies on the ray and is the ray's point nearest to the row
    o, d = M.world_rays(np.where(free[..., None], 0.5, pixels), k, c2w)
    foot, x = targets.numpy().astype(np.float64), xyz.astype(np.float64)[None]
    off = (foot - o) - d * ((foot - o) * d).sum(axis=-1, keepdims=True)
    assert np.abs(off[~free]).max() <= 8 * 2.0 ** -23 * scale
    assert np.abs(((x - foot) * d).sum(axis=-1)[~free]).max() <= 16 * 2.0 ** -23 * scale
    for name, args in (("xyz", (torch.zeros(n, 2), torch.zeros(2, n, 2), torch.zeros(2, 3, 3), torch.zeros(2, 4, 4))),
                       ("coordinates_xy", (torch.zeros(n, 3), torch.zeros(2, n + 1, 2), torch.zeros(2, 3, 3), torch.zeros(2, 4, 4))),
                       ("coordinates_xy", (torch.zeros(n, 3), torch.zeros(n, 2), torch.zeros(2, 3, 3), torch.zeros(2, 4, 4))),
                       ("intrinsics", (torch.zeros(n, 3), torch.zeros(2, n, 2), torch.zeros(1, 3, 3), torch.zeros(2, 4, 4))),
                       ("cam2world", (torch.zeros(n, 3), torch.zeros(2, n, 2), torch.zeros(2, 3, 3), torch.zeros(2, 3, 4)))):
        with pytest.raises(ValueError, match=f"ray_targets: {name} must be fp32"):
            field_volume.ray_targets(*args)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def _cpu_arguments():
    chain = J.chain()
    tw = J.field_twists(chain)
    joints = J.field_joints(chain, J.run(chain), tw)
    n = chain["labels"].shape[0]
    return chain, tw, joints, joints.tree(), torch.zeros(n, 3), torch.from_numpy(chain["labels"]), torch.zeros(2, n, 3), torch.zeros(n, 6)


def test_the_solver_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import (FieldGrid, FieldMetricCommands, FieldPointCloud, cloud_commands_metric,
                                                        solve_commands_metric)
    chain, tw, joints, tree, xyz, labels, targets, information = _cpu_arguments()
    n = xyz.shape[0]
    name = "solve_commands_metric"
    with pytest.raises(ValueError, match=f"{name}: twists must be a FieldTwists"):
        solve_commands_metric(None, xyz, labels, targets, information)
    with pytest.raises(ValueError, match=f"{name}: xyz must be fp32"):
        solve_commands_metric(tw, xyz.double(), labels, targets, information)
    with pytest.raises(ValueError, match=f"{name}: labels must be int32"):
        solve_commands_metric(tw, xyz, labels.long(), targets, information)
    for bad in (targets.double(), targets[0], targets[:, :-1], None):
        with pytest.raises(ValueError, match=f"{name}: targets must be fp32"):
            solve_commands_metric(tw, xyz, labels, bad, information)
    for bad in (information.double(), information[:-1], torch.zeros(n, 3, 3), torch.zeros(3, n, 6), torch.zeros(n, 9), None):
        with pytest.raises(ValueError, match=f"{name}: information must be fp32 \\[{n}, 6\\] or \\[2, {n}, 6\\]"):
            solve_commands_metric(tw, xyz, labels, targets, bad)
    with pytest.raises(ValueError, match=f"{name}: weights must be fp32"):
        solve_commands_metric(tw, xyz, labels, targets, information, weights=torch.ones(n - 1))
    with pytest.raises(ValueError, match=f"{name}: init must be fp32"):
        solve_commands_metric(tw, xyz, labels, targets, information, init=torch.zeros(3))
    with pytest.raises(ValueError, match=f"{name}: lower > upper"):
        solve_commands_metric(tw, xyz, labels, targets, information, lower=0.5, upper=-0.5)
    with pytest.raises(ValueError, match=f"{name}: reg must be"):
        solve_commands_metric(tw, xyz, labels, targets, information, reg=-1.0)
    with pytest.raises(ValueError, match=f"{name}: damping must be"):
        solve_commands_metric(tw, xyz, labels, targets, information, damping=0.0)
    with pytest.raises(ValueError, match=f"{name}: iterations must be an integer"):
        solve_commands_metric(tw, xyz, labels, targets, information, iterations=1001)
    with pytest.raises(ValueError, match=f"{name}: joints and tree come together"):
        solve_commands_metric(tw, xyz, labels, targets, information, joints=joints)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="must live on the device"):
            solve_commands_metric(tw, xyz, labels, targets, information.cuda())
    for q in (information, information.expand(2, n, 6)):
        with pytest.raises(ValueError, match=f"{name}: .*no CPU path"):
            solve_commands_metric(tw, xyz, labels, targets, q, joints=joints, tree=tree, weights=torch.ones(n), reg=0.1, iterations=0)
    cloud = FieldPointCloud(grid=FieldGrid(chain["origin"], chain["step"], chain["dims"]), index=torch.from_numpy(chain["index"]),
                            xyz=xyz, density=torch.ones(n), color=None, jacobian=None, count=torch.tensor([n], dtype=torch.int32))
    with pytest.raises(ValueError, match="cloud_commands_metric: cloud must be a FieldPointCloud"):
        cloud_commands_metric(None, labels, tw, targets, information)
    with pytest.raises(ValueError, match="cloud_commands_metric: information must be fp32"):
        cloud_commands_metric(cloud, labels, tw, targets, information[:-1])
    with pytest.raises(ValueError, match="cloud_commands_metric: .*no CPU path"):
        cloud_commands_metric(cloud, labels, tw, targets, information, joints=joints, tree=tree)
    fit = FieldMetricCommands(**{f: torch.zeros(1) for f in FieldMetricCommands.__dataclass_fields__})
    fit.cost = torch.tensor([4.0, 0.25], dtype=torch.float64)
    assert fit.rms().tolist() == [2.0, 0.5]


def test_the_registration_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import (FieldGrid, FieldPointCloud, cell_grid, cloud_registration_metric,
                                                        register_commands_metric)
    chain, tw, joints, tree, xyz, labels, _, _ = _cpu_arguments()
    n = xyz.shape[0]
    observed, cells = torch.zeros(50, 3), cell_grid((0.0, 0.0, 0.0), (8.0, 8.0, 8.0), 1.0)
    name = "register_commands_metric"
    for bad in (torch.zeros(50, 6).double(), torch.zeros(49, 6), torch.zeros(2, 50, 6), torch.zeros(50, 3, 3), None):
        with pytest.raises(ValueError, match=f"{name}: observed_information must be fp32 \\[50, 6\\] or \\[1, 50, 6\\]"):
            register_commands_metric(tw, xyz, labels, observed, bad, cells, 1.0)
    with pytest.raises(ValueError, match=f"{name}: observed must be fp32"):
        register_commands_metric(tw, xyz, labels, observed.double(), torch.zeros(50, 6), cells, 1.0)
    with pytest.raises(ValueError, match=f"{name}: rounds must be an integer"):
        register_commands_metric(tw, xyz, labels, observed, torch.zeros(50, 6), cells, 1.0, rounds=0)
    with pytest.raises(ValueError, match=f"{name}: max_distance must be a finite number"):
        register_commands_metric(tw, xyz, labels, observed, torch.zeros(50, 6), cells, 0.0)
    for q in (torch.zeros(50, 6), torch.zeros(1, 50, 6)):
        with pytest.raises(ValueError, match=f"{name}: .*no CPU path"):
            register_commands_metric(tw, xyz, labels, observed, q, cells, 1.0, joints=joints, tree=tree)
    with pytest.raises(ValueError, match=f"{name}: .*no CPU path"):
        register_commands_metric(tw, xyz, labels, observed.expand(3, 50, 3), torch.zeros(3, 50, 6), cells, 1.0, init=torch.zeros(3, 3))
    cloud = FieldPointCloud(grid=FieldGrid(chain["origin"], chain["step"], chain["dims"]), index=torch.from_numpy(chain["index"]),
                            xyz=xyz, density=torch.ones(n), color=None, jacobian=None, count=torch.tensor([n], dtype=torch.int32))
    with pytest.raises(ValueError, match="cloud_registration_metric: cloud must be a FieldPointCloud"):
        cloud_registration_metric(None, labels, tw, observed, torch.zeros(50, 6), 1.0)
    with pytest.raises(ValueError, match="cloud_registration_metric: observed_information must be fp32"):
        cloud_registration_metric(cloud, labels, tw, observed, torch.zeros(49, 6), 1.0)
    with pytest.raises(ValueError, match="cloud_registration_metric: cloud.grid must be a FieldGrid"):
        cloud_registration_metric(dataclasses.replace(cloud, grid=None), labels, tw, observed, torch.zeros(50, 6), 1.0)
    with pytest.raises(ValueError, match="cloud_registration_metric: .*no CPU path"):
        cloud_registration_metric(cloud, labels, tw, observed, torch.zeros(50, 6), 1.0, joints=joints, tree=tree)


def test_the_signatures():
    from neural_jacobian_field_amd import field_volume
    keywords = dict(joints=None, tree=None, weights=None, count=None, init=None, lower=None, upper=None, reg=0.0, iterations=20,
                    damping=1e-3)

    def check(fn, positional, keywords):
        params = inspect.signature(fn).parameters
        assert list(params) == positional + list(keywords)
        assert {k: params[k].default for k in keywords} == keywords
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
        assert all(params[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in positional)

    # the keywords are those of the isotropic functions, name for name and default for default
    assert list(keywords) == [k for k, v in inspect.signature(field_volume.solve_commands).parameters.items() if v.kind is v.KEYWORD_ONLY]
    check(field_volume.solve_commands_metric, ["twists", "xyz", "labels", "targets", "information"], keywords)
    cloud = {k: v for k, v in keywords.items() if k != "count"}
    check(field_volume.cloud_commands_metric, ["cloud", "labels", "twists", "targets", "information"], cloud)
    reg = {k: p.default for k, p in inspect.signature(field_volume.register_commands).parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert reg["rounds"] == 8 and reg["iterations"] == 3
    check(field_volume.register_commands_metric, ["twists", "xyz", "labels", "observed", "observed_information", "cells", "max_distance"], reg)
    reg = {k: p.default for k, p in inspect.signature(field_volume.cloud_registration).parameters.items() if p.kind is p.KEYWORD_ONLY}
    check(field_volume.cloud_registration_metric, ["cloud", "labels", "twists", "observed", "observed_information", "max_distance"], reg)
    assert list(inspect.signature(field_volume.ray_targets).parameters) == ["xyz", "coordinates_xy", "intrinsics", "cam2world"]
    assert list(inspect.signature(field_volume.plane_information).parameters) == ["normals"]
    params = inspect.signature(field_volume.ray_information).parameters
    assert list(params) == ["directions", "along"] and params["along"].default == 0.0
    assert list(field_volume.FieldMetricCommands.__dataclass_fields__) == list(field_volume.FieldCommands.__dataclass_fields__)
    assert callable(field_volume.FieldMetricCommands.rms)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "njf_field_commands_metric"
    assert name in declared and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    params = re.search(name + r"\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_commands_metric.argtypes) == ARGUMENTS
    assert len(lib.njf_field_commands.argtypes) == ARGUMENTS - 2
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_COMMANDS_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_COMMANDS_METRIC_MOMENTS_PER_PART"] == hip.FIELD_COMMANDS_METRIC_MOMENTS_PER_PART == M.MOMENTS == 74
    assert defines["NJF_FIELD_COMMANDS_METRIC_BUTTERFLY"] == hip.FIELD_COMMANDS_METRIC_BUTTERFLY == 4
    assert not hip.FIELD_COMMANDS_METRIC_BUTTERFLY & hip.FIELD_COMMANDS_ALL
    assert "NJF_FIELD_COMMANDS_METRIC_WORKSPACE(M, K, A, n)" in header
    assert hip.field_commands_metric_workspace(70, 3, 10, 4097) == (74 * 2 + 120) * 210
    assert hip.field_commands_metric_workspace(1, 256, 1, 0) == 12 * 256


def test_the_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("parts", "parts_count", "num_parts", "part_status", "centroid", "omega", "velocity", "action_dim", "part_a", "part_b",
             "joints_count", "max_joints", "anchor", "joint_omega", "joint_velocity", "parent", "joint_of", "xyz", "labels", "count",
             "n", "targets", "information", "information_per_problem", "num_problems", "weights", "weights_per_problem", "init",
             "lower", "upper", "reg", "iterations", "damping", "commands", "cost", "initial_cost", "weight", "steps", "gradient",
             "status", "out_part_status", "depth", "moments", "workspace", "workspace_doubles", "phases")
    assert len(names) + 1 == ARGUMENTS
    need = hip.field_commands_metric_workspace(5, 4, 8, 5000)
    assert need > hip.field_commands_workspace(5, 4, 8, 5000)

    def call(**kw):
        args = {k: P for k in names}
        args.update(num_parts=4, action_dim=8, max_joints=16, n=5000, information_per_problem=1, num_problems=5, weights_per_problem=1,
                    reg=0.0, iterations=20, damping=1e-3, workspace_doubles=need, phases=3)
        args.update(kw)
        return lib.njf_field_commands_metric(*[args[k] for k in names], None)

    for key, values in (("num_parts", (0, -3, 257)), ("action_dim", (0, -1, 11)), ("num_problems", (0, -1, 65536)),
                        ("max_joints", (0, -1, 4097)), ("phases", (0, -1, 4, 6, 8, 11)), ("iterations", (-1, 1001)),
                        ("damping", (0.0, -1.0, float("nan"))), ("reg", (-1e-9, float("nan"))), ("weights_per_problem", (-1, 2)),
                        ("information_per_problem", (-1, 2))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)
    assert call(n=-1) == E_SHAPE
    assert call(workspace_doubles=need - 1) == E_SHAPE
    assert call(workspace_doubles=hip.field_commands_workspace(5, 4, 8, 5000)) == E_SHAPE       # the isotropic entry's size is too small
    integers = ("num_parts", "action_dim", "max_joints", "n", "information_per_problem", "num_problems", "weights_per_problem", "reg",
                "iterations", "damping", "workspace_doubles", "phases")
    for key in names:
        if key in integers or key in ("parts_count", "joints_count", "count", "weights", "init", "lower", "upper"):
            continue                                                            # (numbers, optional pointers)
        assert call(**{key: None}) == E_NULL, key
    for phases in (1, 3, 5, 7):                                                 # every phase set with the moments needs the information
        assert call(phases=phases, information=None) == E_NULL
    none = dict(part_a=None, part_b=None, joints_count=None, anchor=None, joint_omega=None, joint_velocity=None)
    assert call(**none) == E_NULL                                               # a tree without joints
    assert call(parent=None, joint_of=None) == E_NULL                           # joints without a tree
    assert call(**none, parent=None, joint_of=None, max_joints=0, workspace_doubles=need - 1) == E_SHAPE
    # the moments phase alone needs no solver output, the solver phase alone no rows and no information -- but its outputs
    assert call(phases=1, commands=None, cost=None, moments=None) == E_NULL
    assert call(phases=2, xyz=None, labels=None, targets=None, information=None, status=None) == E_NULL
