"""GPU tests of posing the parts under a command (field_volume.part_poses / cloud_pose / FieldPose.apply; njf_field_pose;
DESIGN.md section 17) against the numpy restatement of its semantics (tests/field_pose_restatement.py).

Transforms: ``|R - R_ref| <= 1e-13 (depth + 1)`` and ``|t - t_ref| <= 1e-13 (depth + 1) max(1, L)``, L the largest magnitude among
the centroid and anchor coordinates and the commanded speeds -- a link is about 100 double operations and two libm calls of
1-2 ulp on either side, under 1e-14; the bound leaves an order of magnitude, and an fp32 evaluation misses it by four.  Status
and depth: equal.  Points: EQUAL BYTES against the restatement's point stage fed the DEVICE's rotation and translation -- no
transcendental and no sum over rows is left there.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_joints_restatement as J
import field_pose_restatement as R

pytestmark = pytest.mark.gpu

IMG = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def chain():
    return J.chain()


@pytest.fixture(scope="module")
def blocks():
    """``blocks()`` with a part count of 53 for its 54 slots -- the last slot is unused although it holds a label, and its rows
    become rows of no part -- and one part without a fitted twist (status EMPTY)."""
    scene = J.blocks()
    assert scene["parts"].shape[0] == 54 and scene["status"][3] == J.TRANSLATION
    scene["parts_count"] = 53
    scene["status"][5] = J.EMPTY
    return scene


@pytest.fixture(scope="module")
def face():
    return J.face()


def _one(dev, v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=dev)


def _grid(scene):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid(scene["origin"], scene["step"], scene["dims"])


def _np(t):
    return t.cpu().numpy()


def _rows(dev, scene, seed=11):
    """(xyz [n, 3] fp32, labels [n] int32, jacobian [n, A, 3] fp32) of a scene's rows, on the device."""
    rng = np.random.default_rng(seed)
    xyz = J.node_coordinates(scene["dims"], scene["index"]).astype(np.float32)
    jac = rng.normal(size=(xyz.shape[0], scene["omega"].shape[1], 3)).astype(np.float32)
    return torch.from_numpy(xyz).to(dev), torch.from_numpy(scene["labels"]).to(dev), torch.from_numpy(jac).to(dev)


def _device_joints(dev, scene, **options):
    from neural_jacobian_field_amd.field_volume import part_joints
    tw = J.field_twists(scene, dev)
    index, labels = torch.from_numpy(scene["index"]).to(dev), torch.from_numpy(scene["labels"]).to(dev)
    return tw, part_joints(_grid(scene), index, labels, tw, batch=scene["batch"], count=_one(dev, scene["count"]), **options)


def _twists_dict(tw):
    return dict(status=_np(tw.status), count=int(tw.count.item()), centroid=_np(tw.centroid), omega=_np(tw.omega),
                velocity=_np(tw.velocity))


def _joints_dict(joints):
    return None if joints is None else dict(part_a=_np(joints.part_a), part_b=_np(joints.part_b), count=int(joints.count.item()),
                                            anchor=_np(joints.anchor), omega=_np(joints.omega), velocity=_np(joints.velocity))


def _commands(m, a, seed=7, scale=1.0):
    return (scale * np.random.default_rng(seed).uniform(-1.0, 1.0, size=(m, a))).astype(np.float32)


def _check_pose(pose, tw, commands, joints=None, tree=None):
    """The device's transforms against the restatement fed the same tensors: the worst ratio to the bound."""
    k, m = tw.labels.shape[0], commands.shape[0]
    for f, shape, dtype in (("rotation", (m, k, 3, 3), torch.float64), ("translation", (m, k, 3), torch.float64),
                            ("status", (k,), torch.int32), ("depth", (k,), torch.int32)):
        t = getattr(pose, f)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cuda", f
    assert pose.labels is tw.labels and pose.count is tw.count
    twd, jd = _twists_dict(tw), _joints_dict(joints)
    tr = None if tree is None else tuple(_np(t) for t in tree)
    ref = R.poses(twd, commands, jd, tr)
    assert np.array_equal(_np(pose.status), ref["status"]) and np.array_equal(_np(pose.depth), ref["depth"])
    ratio = R.worst_ratio(_np(pose.rotation), _np(pose.translation), ref, R.scale_of(twd, commands, jd))
    print(f"transforms: worst ratio to the bound {ratio:.4f} (K = {k}, M = {m}, depth <= {int(ref['depth'].max())})")
    assert ratio <= 1.0
    bad = (ref["status"] & 2) != 0
    assert torch.equal(pose.rotation[:, bad].cpu(), torch.eye(3, dtype=torch.float64).expand(m, int(bad.sum()), 3, 3))
    assert not pose.translation[:, bad].any()
    return ref


def _check_points(pose, commands, xyz, labels, posed, count=None, jacobian=None, sentinel=None):
    """Equal bytes with the restatement's point stage fed the device's transforms."""
    m, n = commands.shape[0], xyz.shape[0]
    assert tuple(posed.shape) == (m, n, 3) and posed.dtype == torch.float32
    out = None if sentinel is None else np.full((m, n, 3), sentinel, np.float32)
    want = R.points(_np(pose.rotation), _np(pose.translation), _np(pose.status), _np(pose.labels), int(pose.count.item()), commands,
                    _np(xyz), _np(labels), count, None if jacobian is None else _np(jacobian), out=out)
    rows = n if count is None else min(max(count, 0), n)
    got = _np(posed)
    assert got[:, :rows].tobytes() == want[:, :rows].tobytes()
    if sentinel is not None:
        assert got.tobytes() == want.tobytes()
    return want


def _cloud(dev, scene, xyz, jacobian):
    from neural_jacobian_field_amd.field_volume import FieldPointCloud
    n = xyz.shape[0]
    return FieldPointCloud(grid=_grid(scene), index=torch.from_numpy(scene["index"]).to(dev), xyz=xyz, density=torch.ones(n, device=dev),
                           color=None, jacobian=jacobian, count=_one(dev, scene["count"]))


# ---- the planted chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 3, 70))
def test_the_planted_chain(dev, chain, m):
    from neural_jacobian_field_amd.field_volume import cloud_pose, part_poses
    tw, joints = _device_joints(dev, chain)
    tree = joints.tree()
    assert all(t.dtype == torch.int32 and t.device == joints.part_a.device for t in tree) and tree[0].tolist() == [-1, 0, 1]
    xyz, labels, jac = _rows(dev, chain)
    assert xyz.shape[0] == 272
    commands = _commands(m, 3, scale=1.4)                        # angles up to 1 and 1.8 rad
    u = torch.from_numpy(commands).to(dev)
    pose, posed = cloud_pose(_cloud(dev, chain, xyz, jac), labels, tw, u, joints=joints, tree=tree)
    ref = _check_pose(pose, tw, commands, joints, tree)
    assert ref["status"].tolist() == [0, 0, 0] and ref["depth"].tolist() == [0, 1, 2]
    _check_points(pose, commands, xyz, labels, posed, jacobian=jac)
    # the base stays where it is, bit for bit; a link's nodes keep their mutual distances to fp32 rounding
    base = labels == int(tw.labels[0])
    assert torch.equal(posed[:, base], xyz[base].expand(m, -1, 3))
    tip = labels == int(tw.labels[2])
    before, after = torch.cdist(xyz[tip].double(), xyz[tip].double()), torch.cdist(posed[0, tip].double(), posed[0, tip].double())
    assert float((before - after).abs().max()) < 1e-5
    # part_poses alone and FieldPose.apply give the same bytes; matrix() holds both
    alone = part_poses(tw, u, joints=joints, tree=tree)
    for f in ("rotation", "translation", "status", "depth"):
        assert torch.equal(getattr(alone, f).view(torch.uint8), getattr(pose, f).view(torch.uint8)), f
    assert torch.equal(alone.apply(xyz, labels, jacobian=jac).view(torch.uint8), posed.view(torch.uint8))
    mat = pose.matrix()
    assert torch.equal(mat[..., :3, :3], pose.rotation) and torch.equal(mat[..., :3, 3], pose.translation)
    assert torch.equal(mat[..., 3, :], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=dev).expand(m, 3, 4))
    # treeless: every part by its own twist about its centroid
    free = part_poses(tw, u)
    _check_pose(free, tw, commands)


# ---- 53 parts and an unused slot: a TRANSLATION and an EMPTY part, unlabelled rows, a label outside the list, padding past count ---------
FORMS = (0, 8, 16, 24)


@pytest.mark.parametrize("with_jacobian", (True, False))
def test_blocks_with_every_kind_of_row(dev, blocks, with_jacobian):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import part_poses
    assert FORMS == (0, hip.FIELD_POSE_STAGED, hip.FIELD_POSE_WIDE, hip.FIELD_POSE_STAGED | hip.FIELD_POSE_WIDE)
    tw, joints = _device_joints(dev, blocks)
    parent, joint_of = joints.parents()                          # int64 on the host
    tree = (parent.to(dev, torch.int32), joint_of.to(dev, torch.int32))
    commands = _commands(3, 4, seed=3)
    u = torch.from_numpy(commands).to(dev)
    pose = part_poses(tw, u, joints=joints, tree=tree)
    ref = _check_pose(pose, tw, commands, joints, tree)
    assert ref["status"][53] == 1 and ref["status"][5] == 1 and ref["status"][3] == 0 and ref["depth"].max() >= 3
    free = part_poses(tw, u)                                     # treeless: the TRANSLATION part (omega = 0) only shifts
    _check_pose(free, tw, commands)
    assert torch.equal(free.rotation[:, 3].cpu(), torch.eye(3, dtype=torch.float64).expand(3, 3, 3)) and free.translation[:, 3].any()
    xyz, labels, jac = _rows(dev, blocks)
    n, count = xyz.shape[0], blocks["count"]
    assert n > count and (n * 12) % 16 != 0                      # padding past the count; the second command's rows start off 16 bytes
    jac = jac if with_jacobian else None
    sentinel = -12345.0
    want = None
    for form in FORMS:
        posed = torch.full((3, n, 3), sentinel, dtype=torch.float32, device=dev)
        points = dict(xyz=xyz, labels=labels, count=_one(dev, count), jacobian=jac, posed=posed)
        hip.field_pose(pose.labels, None, None, None, None, pose.commands,
                       dict(rotation=pose.rotation, translation=pose.translation, status=pose.status, depth=pose.depth),
                       parts_count=pose.count, points=points, phase=hip.FIELD_POSE_POINTS | form)
        want = _check_points(pose, commands, xyz, labels, posed, count=count, jacobian=jac, sentinel=sentinel)
    assert np.all(want[:, count:] == sentinel)
    # the kinds of rows this scene holds, in the restatement's result: rigid rows moved, the others stepped or copied
    slot = J.slots(blocks["labels"], blocks["parts"], blocks["parts_count"], count)
    x = _np(xyz)
    loose = (slot < 0) | (slot == 5)
    loose[count:] = False
    assert (blocks["labels"][:count] == -1).any() and (blocks["labels"][:count] == blocks["outside_label"]).any() and (slot == 5).any()
    if with_jacobian:
        assert (want[0][loose] != x[loose]).any()
    else:
        assert want[0][loose].tobytes() == x[loose].tobytes()
    rigid = (slot >= 0) & (slot != 5)
    assert (want[0][rigid] != x[rigid]).any()
    # the apply method with the count: the same rows
    got = pose.apply(xyz, labels, count=_one(dev, count), jacobian=jac)
    assert _np(got)[:, :count].tobytes() == want[:, :count].tobytes()


# ---- several workgroups, a partial last one, A = 10, every alignment of a command's rows ------------------------------------------------
def test_a_face_of_3240_rows(dev, face):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import cloud_pose, part_poses
    tw, joints = _device_joints(dev, face)
    tree = joints.tree()
    xyz, labels, jac = _rows(dev, face)
    assert xyz.shape[0] == 3240 and jac.shape[1] == 10
    commands = _commands(2, 10, seed=4, scale=0.3)
    u = torch.from_numpy(commands).to(dev)
    pose, posed = cloud_pose(_cloud(dev, face, xyz, jac), labels, tw, u, joints=joints, tree=tree)
    ref = _check_pose(pose, tw, commands, joints, tree)
    assert ref["depth"].max() >= 1 and not ref["status"].any()
    _check_points(pose, commands, xyz, labels, posed, jacobian=jac)
    # one row fewer: commands 1, 2, 3 start 12, 8 and 4 bytes past a 16-byte boundary; every form of the points launch, some rows
    # unlabelled so that both kinds sit in one wave
    n = 3239
    xyz, labels, jac = xyz[:n].contiguous(), labels[:n].clone(), jac[:n].contiguous()
    labels[5::7] = -1
    commands = _commands(4, 10, seed=5, scale=0.3)
    pose = part_poses(tw, torch.from_numpy(commands).to(dev), joints=joints, tree=tree)
    for form in FORMS:
        posed = torch.full((4, n, 3), 7.0, dtype=torch.float32, device=dev)
        points = dict(xyz=xyz, labels=labels, count=None, jacobian=jac, posed=posed)
        hip.field_pose(pose.labels, None, None, None, None, pose.commands,
                       dict(rotation=pose.rotation, translation=pose.translation, status=pose.status, depth=pose.depth),
                       parts_count=pose.count, points=points, phase=hip.FIELD_POSE_POINTS | form)
        _check_points(pose, commands, xyz, labels, posed, jacobian=jac, sentinel=7.0)


# ---- a line of 256 one-node parts: depth 255, the step limit, a cycle ----------------------------------------------------------------------
def _line(dev, joints, tree, scene):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldJoints
    tw = J.field_twists(dict(scene, weight=np.ones(256), energy=np.zeros((256, 3))), dev)
    t = lambda v, dtype: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).to(dev)   # noqa: E731
    j = joints["part_a"].shape[0]
    fj = FieldJoints(grid=FieldGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2)), labels=tw.labels, part_a=t(joints["part_a"], torch.int32),
                     part_b=t(joints["part_b"], torch.int32), contacts=torch.ones(j, dtype=torch.int64, device=dev),
                     status=torch.zeros(j, dtype=torch.int32, device=dev), count=_one(dev, joints["count"]),
                     anchor=t(joints["anchor"], torch.float64), omega=t(joints["omega"], torch.float64),
                     velocity=t(joints["velocity"], torch.float64), twists=tw)
    return tw, fj, tuple(t(v, torch.int32) for v in tree)


def test_a_line_of_256_parts_and_a_cycle(dev):
    from neural_jacobian_field_amd.field_volume import part_poses
    scene, joints, tree = R.line()
    commands = _commands(1, 3, seed=6)
    u = torch.from_numpy(commands).to(dev)
    tw, fj, tr = _line(dev, joints, tree, scene)
    pose = part_poses(tw, u, joints=fj, tree=tr)
    ref = _check_pose(pose, tw, commands, fj, tr)
    assert ref["depth"].tolist() == list(range(256)) and not ref["status"].any()
    xyz = torch.from_numpy(scene["centroid"].astype(np.float32)).to(dev)
    labels = torch.arange(256, dtype=torch.int32, device=dev)
    _check_points(pose, commands, xyz, labels, pose.apply(xyz, labels))
    assert float((pose.translation[0, 255] - pose.translation[0, 0]).abs().max()) > 1e-3        # the tip has moved
    # the same arrays with parent[0] = 255: slot 0 hangs on a joint that does not join it to 255, everything hangs on slot 0
    cyc = (tr[0].clone(), tr[1].clone())
    cyc[0][0] = 255
    pose = part_poses(tw, u, joints=fj, tree=cyc)
    ref = _check_pose(pose, tw, commands, fj, cyc)
    assert (ref["status"] == 2).all()
    # ... and with a joint (0, 255) in a further row, every link is good and only the step limit ends the walk
    closed = {k: np.concatenate([v, v[:1]]) if isinstance(v, np.ndarray) else v for k, v in joints.items()}
    closed["part_a"][255], closed["part_b"][255], closed["count"] = 0, 255, 256
    tw, fj, _ = _line(dev, closed, tree, scene)
    cyc[1][0] = 255
    pose = part_poses(tw, u, joints=fj, tree=cyc)
    ref = _check_pose(pose, tw, commands, fj, cyc)
    assert (ref["status"] == 2).all() and (ref["depth"] == 256).all()
    assert torch.equal(pose.apply(xyz, labels)[0], xyz)                                        # nothing moves


# ---- parts_count above and below K, more joints than rows -----------------------------------------------------------------------------------
def _cut(scene, k, parts_count):
    s = dict(scene)
    for key in ("parts", "status", "centroid", "omega", "velocity", "weight", "energy"):
        s[key] = scene[key][:k]
    s["parts_count"] = parts_count
    return s


def test_truncated_part_and_joint_lists(dev, blocks):
    from neural_jacobian_field_amd.field_volume import part_poses
    commands = _commands(2, 4, seed=8)
    u = torch.from_numpy(commands).to(dev)
    xyz, labels, jac = _rows(dev, blocks)
    count = blocks["count"]
    for scene, options in ((_cut(blocks, 5, 53), {}), (_cut(blocks, 54, 9), {}), (blocks, dict(max_joints=7))):
        tw, joints = _device_joints(dev, scene, **options)
        tree = joints.tree()
        if options:
            assert int(joints.count.item()) > 7 and int(tree[1].max()) < 7
        pose = part_poses(tw, u, joints=joints, tree=tree)
        ref = _check_pose(pose, tw, commands, joints, tree)
        active = min(scene["parts_count"], scene["parts"].shape[0])
        assert (ref["status"][active:] & 1).all()
        posed = pose.apply(xyz, labels, count=_one(dev, count), jacobian=jac)
        _check_points(pose, commands, xyz, labels, posed, count=count, jacobian=jac)
    # a joint count below the stored rows: the slots that hang on the joints past it are bad links
    tw, joints = _device_joints(dev, blocks)
    tree = joints.tree()
    joints.count.fill_(4)
    pose = part_poses(tw, u, joints=joints, tree=tree)
    ref = _check_pose(pose, tw, commands, joints, tree)
    assert (ref["status"] & 2).any() and not (ref["status"] & 2).all()


# ---- determinism and capture -------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_a_capture_replays_them(dev, blocks):
    from neural_jacobian_field_amd.field_volume import cloud_pose
    tw, joints = _device_joints(dev, blocks)
    tree = joints.tree()
    xyz, labels, jac = _rows(dev, blocks)
    cloud = _cloud(dev, blocks, xyz, jac)
    u = torch.from_numpy(_commands(40, 4, seed=9)).to(dev)
    fields = ("rotation", "translation", "status", "depth")
    count = blocks["count"]
    first, second = (cloud_pose(cloud, labels, tw, u, joints=joints, tree=tree) for _ in range(2))
    for f in fields:
        assert torch.equal(getattr(first[0], f).view(torch.uint8), getattr(second[0], f).view(torch.uint8)), f
    assert torch.equal(first[1][:, :count].view(torch.uint8), second[1][:, :count].view(torch.uint8))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pose, posed = cloud_pose(cloud, labels, tw, u, joints=joints, tree=tree)
    for f in fields:
        getattr(pose, f).zero_()
    posed.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(getattr(pose, f).view(torch.uint8), getattr(first[0], f).view(torch.uint8)), f
    assert torch.equal(posed[:, :count].view(torch.uint8), first[1][:, :count].view(torch.uint8))
    assert not posed[:, count:].any()                                                          # the replay wrote no row past the count


# ---- end to end: a model's field, its parts, their twists, their joints, their poses ---------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model
    cfg = model_cfg_from_dict({"action_dim": 8, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                               "action_decoder": {"name": "jacobian_mlp"}})
    m = Model(cfg)
    m.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", 8), seed=0), strict=True)
    return m.to(dev).eval().requires_grad_(False)


def _encoding(batch, dev, seed=1):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    c2w = synthetic.general_pose(7, batch, scale=0.04)
    c2w[0] = torch.eye(4)
    k = synthetic.synthetic_cameras(batch)["ctxt_k_norm"]
    return PixelEncoding(features=synthetic.synthetic_features(batch, IMG, IMG, seed=seed).to(dev), extrinsics=c2w.to(dev),
                         intrinsics=k.to(dev), action=synthetic.synthetic_action(batch, 8).to(dev))


def test_cloud_pose_end_to_end(model, dev):
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_components, cloud_joints, cloud_pose, cloud_twists,
                                                        dominant_joint, extract_field)
    grid = FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), (17, 13, 11))
    enc = _encoding(2, dev)
    head, _ = model.compute_density(grid.points(device=dev)[None].expand(2, -1, 3).contiguous(), enc)
    dense = head.density.reshape(-1).double().cpu()
    cloud = extract_field(model, enc, grid, float(torch.quantile(dense, 0.6)))
    assert cloud.index.shape[0] > 100
    labels, sizes, _ = cloud_components(cloud, keys=dominant_joint(cloud.jacobian))
    tw = cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=2, max_parts=64)
    joints = cloud_joints(cloud, labels, tw, batch=2)
    tree = joints.tree()
    assert int(joints.count.item()) >= 1 and int((tree[0] >= 0).sum()) >= 1
    # commands scaled so that the fastest twist turns by about a radian
    speed = float(torch.linalg.vector_norm(tw.omega, dim=-1).max())
    commands = _commands(5, 8, seed=10, scale=1.0 / max(speed, 1e-6))
    u = torch.from_numpy(commands).to(dev)
    count = int(cloud.count.item())
    for first in (True, False):
        pose, posed = cloud_pose(cloud, labels, tw, u, joints=joints, tree=tree, first_order_elsewhere=first)
        ref = _check_pose(pose, tw, commands, joints, tree)
        _check_points(pose, commands, cloud.xyz, labels, posed, count=count, jacobian=cloud.jacobian if first else None)
    print(f"{count} rows, {int(tw.count.item())} parts, {int(joints.count.item())} joints, depth <= {int(ref['depth'].max())}, "
          f"{int((ref['status'] != 0).sum())} slots of status != 0")
    assert ref["depth"].max() >= 1
