"""Host-side tests of inverse kinematics on the part tree (field_volume.solve_commands / cloud_commands; njf_field_commands;
DESIGN.md section 18): the numpy restatement (tests/field_commands_restatement.py) -- its derivative against central
differences of the pose's restatement, the series of the derivative coefficients, the moment form against sums over the rows,
planted commands, bounds, handles, the regulariser, the empty problem -- and every argument check, raised before any device
work: there is no GPU here; the C ABI's symbol and return codes.

``E_m = sum w (|x~|^2 + |y~|^2)`` over the counted rows is the scale of the moment form's cancellation: the cost is a difference
of sums of that size, so it holds to a multiple of ``2^-53 E / W``."""
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import field_commands_restatement as F
import field_joints_restatement as J
import field_pose_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 45
COST_TOL = 2e-13


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


def _chain_scene():
    chain = J.chain()
    ref = J.run(chain)
    tree = (np.array([-1, 0, 1], np.int32), np.array([-1, 0, 1], np.int32))
    xyz = J.node_coordinates(chain["dims"], chain["index"]).astype(np.float32)
    return dict(scene=chain, twists=R.twists_of(chain), joints=R.joints_of(ref), tree=tree, xyz=xyz, labels=chain["labels"],
                parts=chain["parts"])


@pytest.fixture(scope="module")
def chain():
    return _chain_scene()


@pytest.fixture(scope="module")
def face():
    scene = J.face()
    scene["omega"], scene["velocity"] = 0.3 * scene["omega"], 0.05 * scene["velocity"]
    xyz = J.node_coordinates(scene["dims"], scene["index"]).astype(np.float32)
    return dict(scene=scene, twists=R.twists_of(scene), joints=None, tree=None, xyz=xyz, labels=scene["labels"], parts=scene["parts"])


def _targets(s, commands, **kw):
    return F.posed_targets(s["twists"], np.asarray(commands, np.float32), s["xyz"], s["labels"], s["parts"], s["joints"], s["tree"], **kw)


def _solve(s, targets, **kw):
    return F.solve(s["twists"], s["xyz"], s["labels"], targets, s["parts"], s["joints"], s["tree"], **kw)


def _planted_chain_commands(count, seed=4):
    rng = np.random.default_rng(seed)
    u = np.stack([rng.uniform(-1, 1, count) * 0.98 / 0.7, rng.uniform(-1, 1, count) * 0.98 / 1.3, rng.uniform(-1, 1, count)], axis=1)
    u = u.astype(np.float32)
    assert np.abs(u[:, 0] * 0.7).max() <= 0.98 and np.abs(u[:, 1] * 1.3).max() <= 0.98
    return u


# ---- the derivative ------------------------------------------------------------------------------------------------------------------
def _derivative_error(twists, u, joints, tree, eps=1e-6):
    """The largest difference between ``W x x' + U`` and the central difference of the posed point, over parts and channels; the
    perturbed commands are fp32, so the quotient divides by their true distance."""
    u = np.asarray(u, np.float32)
    here = F.chain(twists, u, joints, tree)
    k = len(here["status"])
    points = np.random.default_rng(0).normal(size=(k, 3))
    worst = 0.0
    for a in range(u.shape[0]):
        up, um = u.copy(), u.copy()
        up[a], um[a] = np.float32(u[a] + eps), np.float32(u[a] - eps)
        ref = R.poses(twists, np.stack([up, um]), joints, tree)
        moved = np.einsum("mkij,kj->mki", ref["rotation"], points) + ref["translation"]
        numeric = (moved[0] - moved[1]) / (float(up[a]) - float(um[a]))
        at = np.einsum("kij,kj->ki", here["rotation"], points) + here["translation"]
        analytic = np.cross(here["twist"][:, a, :3], at) + here["twist"][:, a, 3:]
        worst = max(worst, float(np.abs(numeric - analytic).max()))
    return worst


def test_the_derivative_agrees_with_central_differences(chain, face):
    u = [0.4, -0.6, 0.2]
    worst = [_derivative_error(chain["twists"], u, chain["joints"], chain["tree"])]
    scene, joints, tree = R.line(k=6)
    worst.append(_derivative_error(R.twists_of(scene), np.array(u) * 20.0, joints, tree))       # angles of about 0.5 rad per link
    worst.append(_derivative_error(chain["twists"], u, None, None))                           # treeless
    worst.append(_derivative_error(face["twists"], np.linspace(-0.5, 0.5, 10), None, None))
    print("derivative against central differences:", worst)
    assert max(worst) <= 1e-8
    # the pose inside the chain walk is the pose's restatement
    here = F.chain(chain["twists"], np.float32(u), chain["joints"], chain["tree"])
    ref = R.poses(chain["twists"], np.float32([u]), chain["joints"], chain["tree"])
    assert np.array_equal(here["rotation"], ref["rotation"][0]) and np.array_equal(here["translation"], ref["translation"][0])
    assert np.array_equal(here["status"], ref["status"]) and np.array_equal(here["depth"], ref["depth"])


def test_the_series_of_the_derivative_coefficients_join_the_closed_forms():
    th2 = F.SERIES
    a, b, g = R.coefficients(th2)
    series, closed = F.derivative_coefficients(th2, a, b, g, series=True), F.derivative_coefficients(th2, a, b, g, series=False)
    for s, c in zip(series, closed):
        assert abs(s - c) <= 1e-9 * abs(c)
    assert F.derivative_coefficients(th2, a, b, g) == series
    assert F.derivative_coefficients(np.nextafter(th2, 1.0), a, b, g) == F.derivative_coefficients(np.nextafter(th2, 1.0), a, b, g, series=False)
    # the series against the Taylor sums of db/dth2 and dg/dth2 carried to twelve terms
    for t in (0.0, 1e-3, 5e-3, 1e-2):
        b2, g2 = F.derivative_coefficients(t, *R.coefficients(t), series=True)
        want_b = sum(k * (-1.0) ** k * t ** (k - 1) / math.factorial(2 * k + 2) for k in range(1, 13))
        want_g = sum(k * (-1.0) ** k * t ** (k - 1) / math.factorial(2 * k + 3) for k in range(1, 13))
        dropped = 5.0 * t ** 4 / math.factorial(12)                  # the first term the four-term series leaves out (1e-16 at 1e-2)
        assert abs(b2 - want_b) <= dropped + 1e-16 and abs(g2 - want_g) <= dropped + 1e-16


# ---- the moment form --------------------------------------------------------------------------------------------------------------
def test_the_moment_form_is_the_sum_over_the_rows(chain, face):
    for s, u, at in ((chain, [[0.9, -0.5, 0.3], [0.2, 0.7, 0.0]], [0.3, 0.2, -0.4]),
                     (face, 0.3 * np.random.default_rng(1).uniform(-1, 1, (2, 10)), np.linspace(-0.2, 0.2, 10))):
        targets = _targets(s, u)
        rng = np.random.default_rng(2)
        weights = rng.uniform(0.1, 2.0, size=targets.shape[:2]).astype(np.float32)
        status, _ = F.pose_status(s["twists"], s["joints"], s["tree"])
        mom, _ = F.moments(s["xyz"], s["labels"], targets, s["parts"], None, status, s["twists"]["centroid"], weights)
        slot, w = F.counted(s["xyz"], s["labels"], targets, s["parts"], None, status, weights)
        energy, total = F.energy(mom)
        pose = F.chain(s["twists"], np.float32(at), s["joints"], s["tree"])
        for m in range(targets.shape[0]):
            c0, g0, h0, w0 = F.evaluate_moments(mom[m], pose, s["twists"]["centroid"])
            c1, g1, h1, w1 = F.evaluate_rows(s["xyz"], slot, w[m], targets[m], pose)
            print("moment form:", abs(c0 - c1) / (energy[m] / total[m]), np.abs(g0 - g1).max() / np.abs(g1).max(),
                  np.abs(h0 - h1).max() / np.abs(h1).max())
            assert abs(w0 - w1) <= 1e-12 * w1 and abs(w0 - total[m]) <= 1e-12 * w1
            assert abs(c0 - c1) <= 1e-13 * energy[m] / total[m]
            assert np.abs(g0 - g1).max() <= 1e-12 * np.abs(g1).max() and np.abs(h0 - h1).max() <= 1e-12 * np.abs(h1).max()
            assert np.array_equal(h0, h0.T) or np.abs(h0 - h0.T).max() <= 1e-15 * np.abs(h0).max()


# ---- planted commands ---------------------------------------------------------------------------------------------------------------
def test_planted_commands_on_the_chain_are_recovered(chain):
    planted = _planted_chain_commands(40)
    planted[:, 2] = 0.0
    start = np.zeros((40, 3), np.float32)
    start[:, 2] = np.linspace(-1.0, 1.0, 40, dtype=np.float32)          # channel 2 moves nothing: it must stay where it starts
    out = _solve(chain, _targets(chain, planted), init=start)
    energy, total = F.energy(out["moments"])
    print("chain: steps", out["steps"].max(), "worst cost / (E / W)", (out["cost"] / (energy / total)).max())
    assert not out["status"].any() and (out["cost"] <= COST_TOL * energy / total).all() and (out["cost"] <= out["initial_cost"]).all()
    assert out["commands"][:, 2].tobytes() == start[:, 2].tobytes()
    assert np.abs(out["commands"][:, :2] - planted[:, :2]).max() <= 1e-6
    assert np.abs(out["gradient"]).max() <= 1e-7


@pytest.mark.parametrize("amplitude", (0.05, 0.2, 0.5))
def test_planted_commands_on_the_face_are_recovered(face, amplitude):
    planted = (amplitude * np.random.default_rng(6).uniform(-1, 1, (2, 10))).astype(np.float32)
    out = _solve(face, _targets(face, planted))
    energy, total = F.energy(out["moments"])
    print("face: steps", out["steps"], "cost / (E / W)", out["cost"] / (energy / total))
    assert not out["status"].any() and (out["cost"] <= COST_TOL * energy / total).all()


def test_bounds_hold_and_the_gradient_points_out_of_the_box(chain):
    out = _solve(chain, _targets(chain, [[0.9, -0.7, 0.0]]), lower=-0.5, upper=0.5)
    assert out["commands"].tolist() == [[0.5, -0.5, 0.0]]
    assert out["gradient"][0, 0] < 0.0 and out["gradient"][0, 1] > 0.0 and out["gradient"][0, 2] == 0.0
    per_problem = _solve(chain, _targets(chain, [[0.9, -0.7, 0.0]] * 2), lower=np.float32([[-0.5] * 3, [-2.0] * 3]),
                         upper=np.float32([0.5, 2.0, 2.0]))
    assert per_problem["commands"][0].tolist() == [0.5, -0.5, 0.0]
    second = per_problem["commands"][1]                        # channel 0 on its bound, channel 1 free: it settles where its gradient is 0
    assert second[0] == 0.5 and -2.0 < second[1] < -0.5 and second[2] == 0.0 and abs(per_problem["gradient"][1, 1]) <= 1e-7
    started_outside = _solve(chain, _targets(chain, [[0.1, 0.1, 0.0]]), init=np.float32([[3.0, -3.0, 9.0]]), lower=-0.5, upper=0.5,
                             iterations=0)
    assert started_outside["commands"].tolist() == [[0.5, -0.5, 0.5]] and started_outside["steps"].tolist() == [0]


def test_a_few_handles_recover_the_command(chain):
    planted = np.float32([[0.6, -0.4, 0.0]])
    full = _targets(chain, planted)
    tip = np.flatnonzero(chain["labels"] == chain["parts"][2])
    for rows in (tip[[0, 5, 40, 63]], tip[[17]]):
        targets = np.full_like(full, np.nan)
        targets[:, rows] = full[:, rows]
        out = _solve(chain, targets)
        assert out["weight"].tolist() == [float(len(rows))] and not out["status"].any()
        assert np.abs(out["commands"] - planted).max() <= 1e-5           # one row is three equations for the two moving channels
        energy, total = F.energy(out["moments"])
        assert out["cost"][0] <= COST_TOL * energy[0] / total[0]


def test_the_regulariser_shrinks_the_command(chain):
    targets = _targets(chain, [[0.8, -0.5, 0.0]])
    free, held = _solve(chain, targets), _solve(chain, targets, reg=1e-3)
    assert np.linalg.norm(held["commands"]) < np.linalg.norm(free["commands"]) and held["cost"][0] > free["cost"][0]
    assert np.abs(held["gradient"]).max() <= 1e-7               # the gradient WITH the regulariser vanishes


def test_a_problem_without_rows_keeps_its_clamped_init(chain):
    targets = _targets(chain, [[0.3, 0.3, 0.0]] * 2)
    targets[1] = np.nan
    out = _solve(chain, targets, init=np.float32([[0.0, 0.0, 0.0], [0.2, -3.0, 1.0]]), lower=-1.0, upper=1.0)
    assert out["status"].tolist() == [0, F.NO_ROWS] and out["commands"][1].tolist() == [np.float32(0.2), -1.0, 1.0]
    assert out["cost"][1] == 0.0 and out["weight"][1] == 0.0 and out["steps"][1] == 0 and not out["moments"][1].any()
    zero_weights = _solve(chain, targets[:1], weights=np.zeros(targets.shape[1], np.float32))
    assert zero_weights["status"].tolist() == [F.NO_ROWS]
    with np.errstate(invalid="ignore"):
        not_finite = _solve(chain, targets[:1], init=np.float32([[np.inf, 0.0, 0.0]]))
    assert not_finite["status"].tolist() == [F.NOT_FINITE] and not_finite["steps"].tolist() == [0]


# ---- argument errors ------------------------------------------------------------------------------------------------------------------
def _cpu_arguments():
    chain = J.chain()
    tw = J.field_twists(chain)
    joints = J.field_joints(chain, J.run(chain), tw)
    n = chain["labels"].shape[0]
    return tw, joints, joints.tree(), torch.zeros(n, 3), torch.from_numpy(chain["labels"]), torch.zeros(2, n, 3)


def test_solve_commands_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import solve_commands
    tw, joints, tree, xyz, labels, targets = _cpu_arguments()
    n = xyz.shape[0]
    with pytest.raises(ValueError, match="solve_commands: twists must be a FieldTwists"):
        solve_commands(None, xyz, labels, targets)
    with pytest.raises(ValueError, match="solve_commands: twists.omega must be float64"):
        solve_commands(dataclasses.replace(tw, omega=tw.omega.float()), xyz, labels, targets)
    for bad in (xyz.double(), xyz.reshape(-1), None):
        with pytest.raises(ValueError, match="solve_commands: xyz must be fp32"):
            solve_commands(tw, bad, labels, targets)
    for bad in (labels.long(), labels[:-1]):
        with pytest.raises(ValueError, match="solve_commands: labels must be int32"):
            solve_commands(tw, xyz, bad, targets)
    for bad in (targets.double(), targets[0], targets[:, :-1], torch.zeros(2, n, 2), None):
        with pytest.raises(ValueError, match="solve_commands: targets must be fp32"):
            solve_commands(tw, xyz, labels, bad)
    for m in (0, 65536):
        with pytest.raises(ValueError, match="1 to 65535 target sets"):
            solve_commands(tw, xyz, labels, torch.zeros(m, n, 3))
    for bad in (torch.ones(n).double(), torch.ones(n - 1), torch.ones(3, n), torch.ones(2, n, 1)):
        with pytest.raises(ValueError, match="solve_commands: weights must be fp32"):
            solve_commands(tw, xyz, labels, targets, weights=bad)
    for bad in (torch.zeros(3), torch.zeros(2, 3).double(), torch.zeros(1, 3), np.zeros((2, 3), np.float32)):
        with pytest.raises(ValueError, match="solve_commands: init must be fp32"):
            solve_commands(tw, xyz, labels, targets, init=bad)
    for key in ("lower", "upper"):
        for bad in (torch.zeros(2), torch.zeros(3).double(), torch.zeros(3, 3), "wide"):
            with pytest.raises(ValueError, match=f"solve_commands: {key} must be fp32"):
                solve_commands(tw, xyz, labels, targets, **{key: bad})
    with pytest.raises(ValueError, match="solve_commands: lower > upper"):
        solve_commands(tw, xyz, labels, targets, lower=0.5, upper=-0.5)
    for bad in (-1e-9, float("nan"), "1"):
        with pytest.raises(ValueError, match="solve_commands: reg must be"):
            solve_commands(tw, xyz, labels, targets, reg=bad)
    for bad in (0.0, -1.0, float("nan"), None):
        with pytest.raises(ValueError, match="solve_commands: damping must be"):
            solve_commands(tw, xyz, labels, targets, damping=bad)
    for bad in (-1, 1001, 2.5, True):
        with pytest.raises(ValueError, match="solve_commands: iterations must be an integer"):
            solve_commands(tw, xyz, labels, targets, iterations=bad)
    with pytest.raises(ValueError, match="solve_commands: joints and tree come together"):
        solve_commands(tw, xyz, labels, targets, joints=joints)
    with pytest.raises(ValueError, match="solve_commands: joints must be a FieldJoints"):
        solve_commands(tw, xyz, labels, targets, joints=tw, tree=tree)
    with pytest.raises(ValueError, match="solve_commands: tree (parent|joint_of) must be int32"):
        solve_commands(tw, xyz, labels, targets, joints=joints, tree=joints.parents())
    for bad in (3, torch.ones(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="solve_commands: count must be one int32"):
            solve_commands(tw, xyz, labels, targets, count=bad)
        with pytest.raises(ValueError, match="solve_commands: twists.count must be one int32"):
            solve_commands(dataclasses.replace(tw, count=bad), xyz, labels, targets)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="must live on the device"):
            solve_commands(tw, xyz, labels, targets.cuda())
    for kw in ({}, dict(joints=joints, tree=tree, weights=torch.ones(n), init=torch.zeros(2, 3), lower=-1.0, upper=torch.ones(3),
                        reg=0.1, iterations=0, count=torch.tensor([n], dtype=torch.int32))):
        with pytest.raises(ValueError, match="solve_commands: .*no CPU path"):
            solve_commands(tw, xyz, labels, targets, **kw)


def test_cloud_commands_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldCommands, FieldGrid, FieldPointCloud, cloud_commands
    tw, joints, tree, xyz, labels, targets = _cpu_arguments()
    chain = J.chain()
    n = xyz.shape[0]
    cloud = FieldPointCloud(grid=FieldGrid(chain["origin"], chain["step"], chain["dims"]), index=torch.from_numpy(chain["index"]),
                            xyz=xyz, density=torch.ones(n), color=None, jacobian=None, count=torch.tensor([n], dtype=torch.int32))
    with pytest.raises(ValueError, match="cloud_commands: cloud must be a FieldPointCloud"):
        cloud_commands(None, labels, tw, targets)
    with pytest.raises(ValueError, match="cloud_commands: labels must be int32"):
        cloud_commands(cloud, labels.long(), tw, targets)
    with pytest.raises(ValueError, match="cloud_commands: targets must be fp32"):
        cloud_commands(cloud, labels, tw, targets[:, :-1])
    with pytest.raises(ValueError, match="cloud_commands: count must be one int32"):
        cloud_commands(dataclasses.replace(cloud, count=torch.ones(2, dtype=torch.int32)), labels, tw, targets)
    with pytest.raises(ValueError, match="cloud_commands: .*no CPU path"):
        cloud_commands(cloud, labels, tw, targets, joints=joints, tree=tree)
    fit = FieldCommands(**{f: torch.zeros(1) for f in FieldCommands.__dataclass_fields__})
    fit.cost = torch.tensor([4.0, 0.25], dtype=torch.float64)
    assert fit.rms().tolist() == [2.0, 0.5]


def test_the_pose_keeps_its_messages_after_the_checks_were_factored_out():
    from neural_jacobian_field_amd.field_volume import part_poses
    tw, joints, tree, *_ = _cpu_arguments()
    with pytest.raises(ValueError, match="part_poses: twists.velocity must be float64 \\[3, 3, 3\\]"):
        part_poses(dataclasses.replace(tw, velocity=tw.velocity.float()), torch.zeros(1, 3))
    with pytest.raises(ValueError, match="part_poses: tree parent must be int32 \\[3\\] \\(FieldJoints.tree\\(\\), not parents\\(\\)\\)"):
        part_poses(tw, torch.zeros(1, 3), joints=joints, tree=joints.parents())


def test_the_signatures():
    from neural_jacobian_field_amd import field_volume
    keywords = dict(joints=None, tree=None, weights=None, count=None, init=None, lower=None, upper=None, reg=0.0, iterations=20,
                    damping=1e-3)
    params = inspect.signature(field_volume.solve_commands).parameters
    assert list(params) == ["twists", "xyz", "labels", "targets"] + list(keywords)
    assert {k: params[k].default for k in keywords} == keywords
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    params = inspect.signature(field_volume.cloud_commands).parameters
    del keywords["count"]
    assert list(params) == ["cloud", "labels", "twists", "targets"] + list(keywords)
    assert {k: params[k].default for k in keywords} == keywords
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    assert list(field_volume.FieldCommands.__dataclass_fields__) == ["commands", "cost", "initial_cost", "weight", "steps", "gradient",
                                                                     "status", "part_status", "depth", "moments"]
    assert callable(field_volume.FieldCommands.rms)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "njf_field_commands" in declared and "njf_field_commands" in hip.EXPORTED_SYMBOLS and hasattr(lib, "njf_field_commands")
    params = re.search(r"njf_field_commands\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_commands.argtypes) == ARGUMENTS
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_COMMANDS_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_COMMANDS_ALL"] == hip.FIELD_COMMANDS_ALL == sum(hip.FIELD_COMMANDS_PHASES)
    assert [defines[f"NJF_FIELD_COMMANDS_{n.upper()}"] for n in hip.FIELD_COMMANDS_PHASE_NAMES] == list(hip.FIELD_COMMANDS_PHASES)
    assert defines["NJF_FIELD_COMMANDS_MOMENTS_PER_PART"] == hip.FIELD_COMMANDS_MOMENTS_PER_PART == F.MOMENTS == 23
    assert defines["NJF_FIELD_COMMANDS_MAX_ITERATIONS"] == hip.FIELD_COMMANDS_MAX_ITERATIONS == 1000
    assert (defines["NJF_FIELD_COMMANDS_NO_ROWS"], defines["NJF_FIELD_COMMANDS_NOT_FINITE"]) == (F.NO_ROWS, F.NOT_FINITE) \
        == (hip.FIELD_COMMANDS_NO_ROWS, hip.FIELD_COMMANDS_NOT_FINITE)
    assert "NJF_FIELD_COMMANDS_WORKSPACE(M, K, A, n)" in header
    assert hip.field_commands_workspace(70, 3, 10, 4097) == (23 * 2 + 120) * 210
    assert hip.field_commands_workspace(1, 256, 1, 0) == 12 * 256


def test_the_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("parts", "parts_count", "num_parts", "part_status", "centroid", "omega", "velocity", "action_dim", "part_a", "part_b",
             "joints_count", "max_joints", "anchor", "joint_omega", "joint_velocity", "parent", "joint_of", "xyz", "labels", "count",
             "n", "targets", "num_problems", "weights", "weights_per_problem", "init", "lower", "upper", "reg", "iterations",
             "damping", "commands", "cost", "initial_cost", "weight", "steps", "gradient", "status", "out_part_status", "depth",
             "moments", "workspace", "workspace_doubles", "phases")
    assert len(names) + 1 == ARGUMENTS
    need = hip.field_commands_workspace(5, 4, 8, 5000)

    def call(**kw):
        args = {k: P for k in names}
        args.update(num_parts=4, action_dim=8, max_joints=16, n=5000, num_problems=5, weights_per_problem=1, reg=0.0, iterations=20,
                    damping=1e-3, workspace_doubles=need, phases=3)
        args.update(kw)
        return lib.njf_field_commands(*[args[k] for k in names], None)

    for key, values in (("num_parts", (0, -3, 257)), ("action_dim", (0, -1, 11)), ("num_problems", (0, -1, 65536)),
                        ("max_joints", (0, -1, 4097)), ("phases", (0, -1, 4, 8)), ("iterations", (-1, 1001)),
                        ("damping", (0.0, -1.0, float("nan"))), ("reg", (-1e-9, float("nan"))), ("weights_per_problem", (-1, 2))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)
    assert call(n=-1) == E_SHAPE
    assert call(workspace_doubles=need - 1) == E_SHAPE
    integers = ("num_parts", "action_dim", "max_joints", "n", "num_problems", "weights_per_problem", "reg", "iterations", "damping",
                "workspace_doubles", "phases")
    for key in names:
        if key in integers or key in ("parts_count", "joints_count", "count", "weights", "init", "lower", "upper"):
            continue                                                            # (numbers, optional pointers)
        assert call(**{key: None}) == E_NULL, key
    none = dict(part_a=None, part_b=None, joints_count=None, anchor=None, joint_omega=None, joint_velocity=None)
    assert call(**none) == E_NULL                                               # a tree without joints
    assert call(parent=None, joint_of=None) == E_NULL                           # joints without a tree
    assert call(**none, parent=None, joint_of=None, max_joints=0, workspace_doubles=need - 1) == E_SHAPE
    # the moments phase alone needs no solver output, the solver phase alone no rows -- but its outputs
    assert call(phases=1, commands=None, cost=None, moments=None) == E_NULL
    assert call(phases=2, xyz=None, labels=None, targets=None, status=None) == E_NULL
