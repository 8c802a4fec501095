"""Host-side tests of posing the parts under a command (field_volume.part_poses / cloud_pose / FieldPose; njf_field_pose;
DESIGN.md section 17): the numpy restatement (tests/field_pose_restatement.py) against a Taylor series of the 4 x 4 twist
matrix, the planted 2R arm in closed form, its first-order limit, the treeless mode, trees that are not trees, every argument
check -- raised before any device work: there is no GPU here -- and the C ABI's symbol and return codes.

Tolerances.  A link is about 100 double operations and two libm calls, each within 1-2 ulp (1.1e-16 relative): under 1e-14 on
numbers of magnitude max(1, L), L the largest coordinate or speed that enters.  Comparisons of two evaluations of the same
motion therefore hold to 1e-13 (depth + 1) max(1, L), an order of magnitude above that."""
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_joints_restatement as J
import field_pose_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 33
TOL = 1e-13


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


@pytest.fixture(scope="module")
def chain():
    return J.chain()


@pytest.fixture(scope="module")
def chain_tree(chain):
    """(joints dict, tree) of the chain from the joints' restatement and ``FieldJoints.parents()``."""
    ref = J.run(chain)
    parent, joint_of = J.field_joints(chain, ref, J.field_twists(chain)).parents()
    assert parent.tolist() == [-1, 0, 1] and joint_of.tolist() == [-1, 0, 1]
    return R.joints_of(ref), (parent.numpy().astype(np.int32), joint_of.numpy().astype(np.int32))


def _series(w, v, c, terms=30):
    """exp of the 4 x 4 matrix of the twist (w, v) about c, by its Taylor series."""
    xi = np.zeros((4, 4))
    xi[:3, :3] = R.hat(w)
    xi[:3, 3] = v - R.hat(w) @ c
    out, term = np.eye(4), np.eye(4)
    for i in range(1, terms + 1):
        term = term @ xi / i
        out = out + term
    return out[:3, :3], out[:3, 3]


# ---- the matrix exponential -----------------------------------------------------------------------------------------------------
def test_the_link_motion_is_the_matrix_exponential():
    rng = np.random.default_rng(0)
    thetas = [0.0, 1e-9, 1e-5, 9.9e-4, 0.99999e-3, 1.00001e-3, 1.1e-3, 0.01, 0.3, 1.0, 2.0, 3.0]
    assert any(0 < t * t <= R.SMALL for t in thetas) and any(t * t > R.SMALL for t in thetas)
    for theta in thetas:
        for _ in range(4):
            axis = rng.normal(size=3)
            w = theta * axis / np.linalg.norm(axis)
            v, c = rng.normal(size=3), rng.normal(size=3)
            scale = max(1.0, np.abs(v).max(), np.abs(c).max())
            r, t = R.motion(w, v, c)
            rs, ts = _series(w, v, c)
            # 30 terms: the remainder at theta = 3 is 3^31 / 31! < 1e-19; the series' own rounding is that of ~100 operations
            assert np.abs(r - rs).max() <= TOL and np.abs(t - ts).max() <= TOL * scale, theta
            assert np.abs(r.T @ r - np.eye(3)).max() <= 1e-15, theta
            back = R.compose(R.motion(-w, -v, c), (r, t))
            assert np.abs(back[0] - np.eye(3)).max() <= TOL and np.abs(back[1]).max() <= TOL * scale, theta
    r, t = R.motion(np.zeros(3), [1.0, 2.0, 3.0], [5.0, 5.0, 5.0])                     # a pure translation
    assert np.array_equal(r, np.eye(3)) and np.array_equal(t, [1.0, 2.0, 3.0])


def test_the_coefficients_join_at_the_switch():
    below, above = R.coefficients(R.SMALL), R.coefficients(np.nextafter(R.SMALL, 1.0))
    # a and b are continuous to rounding; g = (th - sin th) / th^3 loses the digits of th - sin th: |dg| <= 2 ulp(th) / th^3
    assert abs(below[0] - above[0]) <= 4e-16 and abs(below[1] - above[1]) <= 4e-16
    assert abs(below[2] - above[2]) <= 2 * np.spacing(1e-3) / 1e-9


# ---- the planted chain in closed form -------------------------------------------------------------------------------------------------
def _rot_z(phi):
    return np.array([[np.cos(phi), -np.sin(phi), 0.0], [np.sin(phi), np.cos(phi), 0.0], [0.0, 0.0, 1.0]])


def _rot_minus_y(phi):
    return np.array([[np.cos(phi), 0.0, -np.sin(phi)], [0.0, 1.0, 0.0], [np.sin(phi), 0.0, np.cos(phi)]])


def _about(r, c):
    return r, c - r @ c


def _hinges():
    o, s = np.asarray(J.ORIGIN, np.float32).astype(np.float64), np.asarray(J.STEP, np.float32).astype(np.float64)
    return [o + s * np.array(c) for c in J.CHAIN_FACE_CENTRES]


def test_the_planted_chain_is_a_2r_arm(chain, chain_tree):
    joints, tree = chain_tree
    commands = np.array([[0.0, 0.0, 0.0], [1.0 / 0.7, 0.0, 5.0], [0.0, -1.0 / 1.3, -2.0], [0.9, 0.6, 1.0], [-1.4, 0.75, 0.0],
                         [1e-4, -1e-4, 3.0]], dtype=np.float32)
    ref = R.poses(R.twists_of(chain), commands, joints, tree)
    assert ref["status"].tolist() == [0, 0, 0] and ref["depth"].tolist() == [0, 1, 2]
    hinge = _hinges()
    scale = max(1.0, np.abs(chain["centroid"]).max(), np.abs(joints["anchor"]).max())
    for m, u in enumerate(commands.astype(np.float64)):
        first = _about(_rot_z(0.7 * u[0]), hinge[0])
        second = _about(_rot_minus_y(1.3 * u[1]), hinge[1])
        both = first[0] @ second[0], first[0] @ second[1] + first[1]
        for p, (r, t) in enumerate(((np.eye(3), np.zeros(3)), first, both)):
            assert np.abs(ref["rotation"][m, p] - r).max() <= TOL * (p + 1), (m, p)
            assert np.abs(ref["translation"][m, p] - t).max() <= TOL * (p + 1) * scale, (m, p)
    assert np.array_equal(ref["rotation"][:, 0], np.broadcast_to(np.eye(3), (len(commands), 3, 3)))   # the base stays, exactly


def test_the_first_order_limit_is_the_twists_jacobian(chain, chain_tree):
    joints, tree = chain_tree
    tw = J.field_twists(chain)
    xyz = J.node_coordinates(chain["dims"], chain["index"])
    slot = J.slots(chain["labels"], chain["parts"])
    u = np.array([0.8, -0.5, 2.0], dtype=np.float32)
    turn = abs(u[0]) * 0.7 + abs(u[1]) * 1.3                                       # |omega| summed along the chain
    reach = max(np.abs(xyz - h).sum(axis=1).max() for h in _hinges())
    errors = []
    for eps in (2.0 ** -6, 2.0 ** -9, 2.0 ** -12):
        ref = R.poses(R.twists_of(chain), (eps * u)[None], joints, tree)
        worst = 0.0
        for p in range(3):
            x = xyz[slot == p]
            moved = x @ ref["rotation"][0, p].T + ref["translation"][0, p]
            first = (tw.jacobian_at(torch.from_numpy(x), p).numpy() * u.astype(np.float64)[None, :, None]).sum(axis=1)
            worst = max(worst, np.abs((moved - x) / eps - first).max())
        # the second-order remainder of a product of exponentials: at most (eps * turn)^2 * reach, divided by eps; 1e-16 / eps
        # of rounding is far below it for these eps
        assert worst <= eps * turn * turn * reach, (eps, worst)
        errors.append(worst)
    assert errors[0] > errors[1] > errors[2] > 0.0


def test_without_a_tree_every_part_moves_by_its_own_twist(chain):
    commands = np.array([[0.5, 1.0, -2.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    ref = R.poses(R.twists_of(chain), commands)
    assert not ref["status"].any() and not ref["depth"].any()
    for m, u in enumerate(commands.astype(np.float64)):
        for p in range(3):
            w, v = (u[:, None] * chain["omega"][p]).sum(axis=0), (u[:, None] * chain["velocity"][p]).sum(axis=0)
            r, t = _series(w, v, chain["centroid"][p])
            assert np.abs(ref["rotation"][m, p] - r).max() <= TOL and np.abs(ref["translation"][m, p] - t).max() <= TOL
    # an empty part and a slot past the count stay, with bit 1; a translation-only part moves by its velocity
    status = np.array([0, 1, 2], np.int32)
    ref = R.poses(R.twists_of(chain, status=status, parts_count=2), commands)
    assert ref["status"].tolist() == [0, 1, 1]
    assert np.array_equal(ref["rotation"][:, 1:], np.broadcast_to(np.eye(3), (2, 2, 3, 3))) and not ref["translation"][:, 1:].any()


# ---- trees that are not trees -----------------------------------------------------------------------------------------------------------
def test_bad_trees_give_the_identity_bit_two_and_a_bounded_walk():
    scene, joints, tree = R.line(k=6)
    commands = np.array([[1.0, 2.0, -1.0]], dtype=np.float32)
    good = R.poses(R.twists_of(scene), commands, joints, tree)
    assert not good["status"].any() and good["depth"].tolist() == [0, 1, 2, 3, 4, 5]
    identity = np.eye(3)

    def run(parent=None, joint_of=None, **kw):
        t = (tree[0].copy() if parent is None else np.array(parent, np.int32),
             tree[1].copy() if joint_of is None else np.array(joint_of, np.int32))
        jo = dict(joints)
        jo.update({k: v for k, v in kw.items() if k in jo})
        tw = R.twists_of(scene, **{k: v for k, v in kw.items() if k not in jo})
        out = R.poses(tw, commands, jo, t)
        assert (out["depth"] <= 6).all()
        for p in range(6):
            if out["status"][p] & 2:
                assert np.array_equal(out["rotation"][0, p], identity) and not out["translation"][0, p].any(), p
        return out

    # a two-cycle 0 <-> 1 (joint 0 joins them): everything hangs on it
    out = run(parent=[1, 0, 1, 2, 3, 4], joint_of=[0, 0, 1, 2, 3, 4])
    assert (out["status"] == 2).all() and out["depth"].max() == 6
    # a self-parent: slot 2 and what hangs on it; slots 0 and 1 keep their poses
    out = run(parent=[-1, 0, 2, 2, 3, 4])
    assert out["status"].tolist() == [0, 0, 2, 2, 2, 2]
    assert np.array_equal(out["rotation"][:, :2], good["rotation"][:, :2])
    # a joint_of that joins other parts
    out = run(joint_of=[-1, 0, 3, 2, 3, 4])
    assert out["status"].tolist() == [0, 0, 2, 2, 2, 2]
    # a parent past the used slots (slot 4 is unused itself, but its parent is a used one)
    out = run(parts_count=4)
    assert out["status"].tolist() == [0, 0, 0, 0, 1, 1 | 2]
    # a joint past the stored ones
    out = run(count=3)
    assert out["status"].tolist() == [0, 0, 0, 0, 2, 2]
    out = run(joint_of=[-1, 0, -1, 2, 3, 7])
    assert out["status"].tolist() == [0, 0, 2, 2, 2, 2]
    # a parent outside [-1, K): -5 makes slot 2 a root for its link, but its walk, and that of what hangs on it, leaves the range
    out = run(parent=[-1, 0, -5, 2, 9, 4])
    assert out["status"].tolist() == [0, 0, 2, 2, 2, 2]
    # the other end of the joint as parent: the sign flips, the motion is the inverse link
    back = run(parent=[1, -1, 1, 2, 3, 4], joint_of=[0, -1, 1, 2, 3, 4])
    assert not back["status"].any() and back["depth"].tolist() == [1, 0, 1, 2, 3, 4]


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
def _cpu_pose(chain, m=2):
    from neural_jacobian_field_amd.field_volume import FieldPose
    tw = J.field_twists(chain)
    return FieldPose(labels=tw.labels, count=tw.count, rotation=torch.eye(3, dtype=torch.float64).expand(m, 3, 3, 3).contiguous(),
                     translation=torch.zeros(m, 3, 3, dtype=torch.float64), status=torch.zeros(3, dtype=torch.int32),
                     depth=torch.zeros(3, dtype=torch.int32), commands=torch.zeros(m, 3))


def test_part_poses_checks_its_arguments_before_any_gpu_work(chain):
    from neural_jacobian_field_amd.field_volume import part_poses
    tw = J.field_twists(chain)
    joints = J.field_joints(chain, J.run(chain), tw)
    tree = joints.tree()
    assert all(t.dtype == torch.int32 and t.device == joints.part_a.device for t in tree)
    assert tree[0].tolist() == [-1, 0, 1] and tree[1].tolist() == [-1, 0, 1] and joints.tree(root=2)[0].tolist() == [1, 2, -1]
    u = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="twists must be a FieldTwists"):
        part_poses(None, u)
    with pytest.raises(ValueError, match="twists.labels must be int32"):
        part_poses(dataclasses.replace(tw, labels=tw.labels.long()), u)
    for k in (0, 257):
        with pytest.raises(ValueError, match="1 to 256 parts"):
            part_poses(dataclasses.replace(tw, labels=torch.zeros(k, dtype=torch.int32)), u)
    for bad in (tw.omega.float(), tw.omega[:2], tw.omega.reshape(3, 9), tw.omega[:, :, :2]):
        with pytest.raises(ValueError, match="twists.omega must be float64"):
            part_poses(dataclasses.replace(tw, omega=bad), u)
    for a in (0, 11):
        with pytest.raises(ValueError, match="1 to 10 command channels"):
            part_poses(dataclasses.replace(tw, omega=torch.zeros(3, a, 3, dtype=torch.float64)), torch.zeros(4, a))
    for field, bad in (("velocity", tw.velocity[:, :2]), ("velocity", tw.velocity.float()), ("centroid", tw.centroid[:2]),
                       ("centroid", tw.centroid.float()), ("status", tw.status.long()), ("status", tw.status[:1])):
        with pytest.raises(ValueError, match=f"twists.{field} must be"):
            part_poses(dataclasses.replace(tw, **{field: bad}), u)
    for bad in (u.double(), torch.zeros(4, 2), torch.zeros(12), None, u.numpy()):
        with pytest.raises(ValueError, match="commands must be fp32"):
            part_poses(tw, bad)
    for m in (0, 65536):
        with pytest.raises(ValueError, match="1 to 65535 commands"):
            part_poses(tw, torch.zeros(m, 3))
    with pytest.raises(ValueError, match="joints and tree come together"):
        part_poses(tw, u, joints=joints)
    with pytest.raises(ValueError, match="joints and tree come together"):
        part_poses(tw, u, tree=tree)
    with pytest.raises(ValueError, match="joints must be a FieldJoints"):
        part_poses(tw, u, joints=tw, tree=tree)
    with pytest.raises(ValueError, match="joints.part_a must be int32"):
        part_poses(tw, u, joints=dataclasses.replace(joints, part_a=joints.part_a.long()), tree=tree)
    for j in (0, 4097):
        with pytest.raises(ValueError, match="1 to 4096 rows"):
            part_poses(tw, u, joints=dataclasses.replace(joints, part_a=torch.zeros(j, dtype=torch.int32)), tree=tree)
    for field, bad in (("part_b", joints.part_b[:5]), ("anchor", joints.anchor.float()), ("omega", joints.omega[:, :2]),
                       ("velocity", joints.velocity[:7])):
        with pytest.raises(ValueError, match=f"joints.{field} must be"):
            part_poses(tw, u, joints=dataclasses.replace(joints, **{field: bad}), tree=tree)
    with pytest.raises(ValueError, match="tree must be"):
        part_poses(tw, u, joints=joints, tree=tree[0])
    for bad in (joints.parents(), (tree[0][:2], tree[1]), (tree[0], tree[1].reshape(3, 1))):   # parents() is int64
        with pytest.raises(ValueError, match="tree (parent|joint_of) must be int32"):
            part_poses(tw, u, joints=joints, tree=bad)
    for bad in (3, torch.ones(2, dtype=torch.int32), torch.ones(1)):
        with pytest.raises(ValueError, match="twists.count must be one int32"):
            part_poses(dataclasses.replace(tw, count=bad), u)
        with pytest.raises(ValueError, match="joints.count must be one int32"):
            part_poses(tw, u, joints=dataclasses.replace(joints, count=bad), tree=tree)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="must live on the device"):
            part_poses(tw, u.cuda())
    for kw in ({}, dict(joints=joints, tree=tree)):
        with pytest.raises(ValueError, match="part_poses: .*no CPU path"):
            part_poses(tw, u, **kw)


def test_cloud_pose_and_apply_check_their_arguments_before_any_gpu_work(chain):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud, cloud_pose
    grid = FieldGrid(chain["origin"], chain["step"], chain["dims"])
    index, labels = torch.from_numpy(chain["index"]), torch.from_numpy(chain["labels"])
    n = index.shape[0]
    cloud = FieldPointCloud(grid=grid, index=index, xyz=torch.zeros(n, 3), density=torch.ones(n), color=None,
                            jacobian=torch.zeros(n, 3, 3), count=torch.tensor([n], dtype=torch.int32))
    tw = J.field_twists(chain)
    u = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="cloud must be a FieldPointCloud"):
        cloud_pose(None, labels, tw, u)
    with pytest.raises(ValueError, match="cloud_pose: labels must be int32"):
        cloud_pose(cloud, labels[:-1], tw, u)
    with pytest.raises(ValueError, match="cloud_pose: commands must be fp32"):
        cloud_pose(cloud, labels, tw, u.double())
    with pytest.raises(ValueError, match="cloud_pose: xyz must be fp32"):
        cloud_pose(dataclasses.replace(cloud, xyz=cloud.xyz.double()), labels, tw, u)
    with pytest.raises(ValueError, match="cloud_pose: jacobian must be fp32"):
        cloud_pose(dataclasses.replace(cloud, jacobian=torch.zeros(n, 2, 3)), labels, tw, u)
    with pytest.raises(ValueError, match="cloud_pose: joints and tree come together"):
        cloud_pose(cloud, labels, tw, u, tree=(torch.zeros(3, dtype=torch.int32),) * 2)
    for first in (True, False):
        with pytest.raises(ValueError, match="cloud_pose: .*no CPU path"):
            cloud_pose(cloud, labels, tw, u, first_order_elsewhere=first)
    # FieldPose.apply
    pose = _cpu_pose(chain)
    xyz = torch.zeros(n, 3)
    for bad in (xyz.double(), xyz.reshape(-1), torch.zeros(n, 2), None):
        with pytest.raises(ValueError, match="FieldPose.apply: xyz must be fp32"):
            pose.apply(bad, labels)
    for bad in (labels.long(), labels[:-1], None):
        with pytest.raises(ValueError, match="FieldPose.apply: labels must be int32"):
            pose.apply(xyz, bad)
    for bad in (torch.zeros(n, 3, 3, dtype=torch.float64), torch.zeros(n, 4, 3), torch.zeros(n - 1, 3, 3)):
        with pytest.raises(ValueError, match="FieldPose.apply: jacobian must be fp32"):
            pose.apply(xyz, labels, jacobian=bad)
    for bad in (3, torch.ones(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="FieldPose.apply: count must be one int32"):
            pose.apply(xyz, labels, count=bad)
    with pytest.raises(ValueError, match="FieldPose.apply: .*no CPU path"):
        pose.apply(xyz, labels, jacobian=torch.zeros(n, 3, 3), count=torch.tensor([n], dtype=torch.int32))
    # matrix() is plain torch
    mat = pose.matrix()
    assert tuple(mat.shape) == (2, 3, 4, 4) and torch.equal(mat, torch.eye(4, dtype=torch.float64).expand(2, 3, 4, 4))


def test_the_signatures():
    from neural_jacobian_field_amd import field_volume
    params = inspect.signature(field_volume.part_poses).parameters
    assert list(params) == ["twists", "commands", "joints", "tree"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None for k in ("joints", "tree"))
    params = inspect.signature(field_volume.cloud_pose).parameters
    assert list(params) == ["cloud", "labels", "twists", "commands", "joints", "tree", "first_order_elsewhere"]
    defaults = dict(joints=None, tree=None, first_order_elsewhere=True)
    assert {k: params[k].default for k in defaults} == defaults
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in defaults)
    params = inspect.signature(field_volume.FieldPose.apply).parameters
    assert list(params) == ["self", "xyz", "labels", "count", "jacobian"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None for k in ("count", "jacobian"))
    assert list(field_volume.FieldPose.__dataclass_fields__) == ["labels", "count", "rotation", "translation", "status", "depth",
                                                                 "commands"]
    assert list(inspect.signature(field_volume.FieldJoints.tree).parameters) == ["self", "root"]


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "njf_field_pose" in declared and "njf_field_pose" in hip.EXPORTED_SYMBOLS and hasattr(lib, "njf_field_pose")
    params = re.search(r"njf_field_pose\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_pose.argtypes) == ARGUMENTS
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_POSE_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_POSE_MAX_COMMANDS"] == hip.FIELD_POSE_MAX_COMMANDS == 65535
    assert defines["NJF_FIELD_POSE_ALL"] == hip.FIELD_POSE_ALL == sum(hip.FIELD_POSE_PHASES)
    assert [defines[f"NJF_FIELD_POSE_{n.upper()}"] for n in hip.FIELD_POSE_PHASE_NAMES] == list(hip.FIELD_POSE_PHASES)
    assert defines["NJF_FIELD_POSE_STAGED"] == hip.FIELD_POSE_STAGED == 8 and defines["NJF_FIELD_POSE_WIDE"] == hip.FIELD_POSE_WIDE == 16
    assert "NJF_FIELD_POSE_WORKSPACE(M, K)" in header
    assert hip.field_pose_workspace(70, 3) == 12 * 210 + 2 and hip.field_pose_workspace(1, 256) == 12 * 256 + 128


def test_the_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("parts", "parts_count", "num_parts", "part_status", "centroid", "omega", "velocity", "action_dim", "part_a", "part_b",
             "joints_count", "max_joints", "anchor", "joint_omega", "joint_velocity", "parent", "joint_of", "commands",
             "num_commands", "rotation", "translation", "status", "depth", "xyz", "labels", "count", "n", "jacobian", "posed",
             "workspace", "workspace_doubles", "phases")
    assert len(names) + 1 == ARGUMENTS
    need = hip.field_pose_workspace(5, 4)

    def call(**kw):
        args = {k: P for k in names}
        args.update(num_parts=4, action_dim=8, max_joints=16, num_commands=5, n=500, workspace_doubles=need, phases=7)
        args.update(kw)
        return lib.njf_field_pose(*[args[k] for k in names], None)

    for bad in (0, -3, 257):
        assert call(num_parts=bad) == E_VALUE
    for bad in (0, -1, 11):
        assert call(action_dim=bad) == E_VALUE
    for bad in (0, -1, 65536):
        assert call(num_commands=bad) == E_VALUE
    for bad in (0, -1, 4097):
        assert call(max_joints=bad) == E_VALUE
    for bad in (0, -1, 32, 64):
        assert call(phases=bad) == E_VALUE
    assert call(n=-1) == E_SHAPE
    assert call(workspace_doubles=need - 1) == E_SHAPE                            # the workspace is too small
    integers = ("num_parts", "action_dim", "max_joints", "num_commands", "n", "workspace_doubles", "phases")
    for key in names:
        if key in integers or key in ("parts_count", "joints_count", "count", "jacobian"):
            continue                                                            # (integers, optional pointers)
        assert call(**{key: None}) == E_NULL, key
    # joints without a tree, a tree without joints
    none = dict(part_a=None, part_b=None, joints_count=None, anchor=None, joint_omega=None, joint_velocity=None)
    assert call(**none) == E_NULL
    assert call(parent=None, joint_of=None) == E_NULL
    # without joints max_joints is not read; the points launch alone needs no twists and no workspace, but its outputs
    assert call(**none, parent=None, joint_of=None, max_joints=0, workspace_doubles=need - 1) == E_SHAPE
    assert call(phases=4, part_status=None, centroid=None, omega=None, velocity=None, workspace=None, workspace_doubles=0,
                posed=None) == E_NULL
