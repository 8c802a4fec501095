"""GPU tests of the joints between parts (field_volume.part_joints / cloud_joints; njf_field_joints)
against the numpy restatement of its semantics (tests/field_joints_restatement.py): EQUAL BYTES for every output -- the integer
lists and the float64 anchors and twists.  No tolerance: the contact table is integer, and no floating-point sum runs over
rows, so numpy's element-wise IEEE arithmetic in the stated order is the device's.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_joints_restatement as R

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
    return R.chain()


@pytest.fixture(scope="module")
def blocks():
    return R.blocks()


@pytest.fixture(scope="module")
def face():
    return R.face()


def _one(dev, v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=dev)


def _grid(scene):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid(scene["origin"], scene["step"], scene["dims"])


def _joints(dev, scene, **options):
    from neural_jacobian_field_amd.field_volume import part_joints
    tw = R.field_twists(scene, dev)
    index, labels = torch.from_numpy(scene["index"]).to(dev), torch.from_numpy(scene["labels"]).to(dev)
    joints = part_joints(_grid(scene), index, labels, tw, batch=scene["batch"], count=_one(dev, scene["count"]), **options)
    j, a = options.get("max_joints", 256), scene["omega"].shape[1]
    shapes = dict(part_a=(j,), part_b=(j,), contacts=(j,), status=(j,), count=(1,), anchor=(j, 3), omega=(j, a, 3), velocity=(j, a, 3))
    for f, shape in shapes.items():
        t = getattr(joints, f)
        want = torch.int64 if f == "contacts" else torch.float64 if f in ("anchor", "omega", "velocity") else torch.int32
        assert tuple(t.shape) == shape and t.dtype == want and t.device.type == "cuda", f
    assert joints.labels is tw.labels and joints.twists is tw
    return joints


def _same_bytes(joints, ref):
    for f in R.OUTPUTS:
        got = getattr(joints, f).cpu().numpy()
        assert got.dtype == ref[f].dtype and got.shape == ref[f].shape, f
        assert got.tobytes() == ref[f].tobytes(), (f, got, ref[f])


def _check(dev, scene, **options):
    ref = R.run(scene, **options)
    joints = _joints(dev, scene, **options)
    _same_bytes(joints, ref)
    return joints, ref


def _cut(scene, k, parts_count=None):
    """The scene with a part list of k slots: the first k parts, or all of them and -1 slots behind."""
    s = dict(scene)
    have = scene["parts"].shape[0]
    for key in ("parts", "status", "centroid", "omega", "velocity", "weight", "energy"):
        v = scene[key][:k]
        if k > have:
            fill = -1 if key == "parts" else 0
            v = np.concatenate([v, np.full((k - have,) + v.shape[1:], fill, dtype=v.dtype)])
        s[key] = v
    s["parts_count"] = parts_count
    return s


# ---- the planted chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", (6, 14))
def test_the_planted_chain(dev, chain, connectivity):
    joints, ref = _check(dev, chain, connectivity=connectivity)
    assert int(joints.count.item()) == 2 and joints.part_a[:2].tolist() == [0, 1] and joints.part_b[:2].tolist() == [1, 2]
    assert joints.contacts[:2].tolist() == ([16, 16] if connectivity == 6 else [64, 49])
    assert joints.drive()[:2].tolist() == [0, 1]
    parent, joint_of = joints.parents()
    assert parent.tolist() == [-1, 0, 1] and joint_of.tolist() == [-1, 0, 1]
    # the methods are plain torch: the device's result and a CPU copy agree
    cpu = R.field_joints(chain, ref, R.field_twists(chain))
    for got, want in zip(joints.screw(), cpu.screw()):
        assert torch.equal(got.cpu().isnan(), want.isnan()) and torch.allclose(got.cpu().nan_to_num(), want.nan_to_num(), atol=1e-12)


# ---- grid faces, batch elements, unlabelled rows, labels outside the list, padding, a single-row part, a status bit -------------------
@pytest.mark.parametrize("connectivity", (6, 14))
def test_blocks_that_touch_every_face_and_both_batch_elements(dev, blocks, connectivity):
    joints, ref = _check(dev, blocks, connectivity=connectivity)
    count = int(joints.count.item())
    assert 50 < count < 256
    nodes = R.BLOCK_DIMS[0] * R.BLOCK_DIMS[1] * R.BLOCK_DIMS[2]
    element = blocks["parts"] // nodes
    a, b = joints.part_a[:count].cpu().numpy(), joints.part_b[:count].cpu().numpy()
    assert (a < b).all() and (element[a] == element[b]).all()                     # nothing joins the two batch elements
    assert (np.diff(a.astype(np.int64) * 256 + b) > 0).all()                        # ascending (lo, hi)
    # the single-row part has joints, and the TRANSLATION bit of part 3 passes through to its joints and to no other
    single = int(np.flatnonzero(blocks["parts"] == blocks["single"])[0])
    assert ((a == single) | (b == single)).any()
    status = joints.status[:count].cpu().numpy()
    assert np.array_equal(status != 0, (a == 3) | (b == 3)) and (status[status != 0] == R.TRANSLATION).all()


def test_more_parts_than_slots_and_fewer(dev, blocks):
    true = blocks["parts"].shape[0]
    # five slots for all the parts: the surplus parts take no part
    joints, ref = _check(dev, _cut(blocks, 5, parts_count=true))
    assert 0 < int(joints.count.item()) <= 10 and int(joints.part_b.max()) < 5
    # 64 slots, the true count: the -1 slots behind it hold nothing; and a count below the parts cuts the list
    _check(dev, _cut(blocks, 64, parts_count=true))
    joints, _ = _check(dev, _cut(blocks, 64, parts_count=9))
    assert int(joints.part_b.max()) < 9
    joints, _ = _check(dev, _cut(blocks, 1))
    assert int(joints.count.item()) == 0 and (joints.part_a == -1).all()


def test_more_joints_than_rows_and_the_contact_threshold(dev, blocks):
    full = R.run(blocks)
    joints, ref = _check(dev, blocks, max_joints=7)
    assert int(joints.count.item()) == full["count"][0] > 7                         # the true count, the first seven stored
    assert np.array_equal(ref["part_a"], full["part_a"][:7]) and np.array_equal(ref["contacts"], full["contacts"][:7])
    _check(dev, blocks, max_joints=1)
    _check(dev, blocks, max_joints=4096, connectivity=14)
    few = full["contacts"][:full["count"][0]]
    assert few.min() < 3 <= few.max()
    joints, ref = _check(dev, blocks, min_contacts=3)
    assert int(joints.count.item()) == int((few >= 3).sum()) < full["count"][0]
    joints, _ = _check(dev, blocks, min_contacts=10 ** 6)
    assert int(joints.count.item()) == 0


# ---- one face of 1,600 contacts: the in-wave combination, several workgroups on one pair ---------------------------------------------
@pytest.mark.parametrize("connectivity", (6, 14))
def test_one_face_of_1600_contacts(dev, face, connectivity):
    joints, ref = _check(dev, face, connectivity=connectivity)
    assert int(joints.count.item()) == 2 and face["index"].shape[0] == 2 * R.FACE * R.FACE + R.FACE
    if connectivity == 6:
        assert joints.contacts[:2].tolist() == [R.FACE * R.FACE, R.FACE]


def test_the_per_lane_form_fills_the_same_table(dev, face, blocks):
    from neural_jacobian_field_amd import hip
    for scene, connectivity in ((face, 6), (face, 14), (blocks, 14)):
        ref = R.run(scene, connectivity=connectivity)
        tw = R.field_twists(scene, dev)
        index, labels = torch.from_numpy(scene["index"]).to(dev), torch.from_numpy(scene["labels"]).to(dev)
        j, a, k = 256, scene["omega"].shape[1], scene["parts"].shape[0]
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        total = scene["batch"] * scene["dims"][0] * scene["dims"][1] * scene["dims"][2]
        for form in (0, hip.FIELD_JOINTS_PER_LANE):
            out = dict(part_a=torch.empty(j, **i32), part_b=torch.empty(j, **i32), contacts=torch.empty(j, dtype=torch.int64, device=dev),
                       status=torch.empty(j, **i32), count=torch.empty(1, **i32), anchor=torch.empty(j, 3, **f64),
                       omega=torch.empty(j, a, 3, **f64), velocity=torch.empty(j, a, 3, **f64))
            workspace = torch.empty(hip.field_joints_workspace(total, k), dtype=torch.int64, device=dev)
            hip.field_joints(_grid(scene).c_grid(), scene["batch"], index, labels, tw.labels, tw.status, tw.centroid, tw.omega,
                             tw.velocity, out, count=_one(dev, scene["count"]), parts_count=tw.count, connectivity=connectivity,
                             phase=hip.FIELD_JOINTS_ALL | form, workspace=workspace)
            for f in R.OUTPUTS:
                assert out[f].cpu().numpy().tobytes() == ref[f].tobytes(), (form, f)
            # the raw table in the workspace: contacts and sum2 per (lo, hi)
            table = workspace[:4 * k * k].cpu().numpy().reshape(k, k, 4)
            assert np.array_equal(table[:, :, 0], ref["table"][0]) and np.array_equal(table[:, :, 1:], ref["table"][1])
            volume = workspace[4 * k * k:].view(torch.int32)[:total].cpu().numpy()
            slot = R.slots(scene["labels"], scene["parts"], None, scene["count"])
            listed = (scene["index"] >= 0) & (scene["index"] < total) & (slot >= 0)
            want = np.full(total, -1, dtype=np.int32)
            want[scene["index"][listed]] = slot[listed]
            assert np.array_equal(volume, want)


# ---- determinism and capture -----------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_a_capture_replays_them(dev, blocks, face):
    from neural_jacobian_field_amd.field_volume import FieldPointCloud, cloud_joints
    first, second = (_joints(dev, face, connectivity=14) for _ in range(2))
    for f in R.OUTPUTS:
        assert torch.equal(getattr(first, f).view(torch.uint8), getattr(second, f).view(torch.uint8)), f
    # cloud_joints on one stream: an eager call, then a capture of the same call
    n = blocks["index"].shape[0]
    cloud = FieldPointCloud(grid=_grid(blocks), index=torch.from_numpy(blocks["index"]).to(dev), xyz=torch.zeros(n, 3, device=dev),
                            density=torch.ones(n, device=dev), color=None, jacobian=None, count=_one(dev, blocks["count"]))
    labels, tw = torch.from_numpy(blocks["labels"]).to(dev), R.field_twists(blocks, dev)
    kw = dict(batch=2, connectivity=14, min_contacts=2)
    eager = cloud_joints(cloud, labels, tw, **kw)
    _same_bytes(eager, R.run(blocks, connectivity=14, min_contacts=2))
    assert int(eager.count.item()) > 20
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = cloud_joints(cloud, labels, tw, **kw)
    for f in R.OUTPUTS:
        getattr(captured, f).zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f in R.OUTPUTS:
        assert torch.equal(getattr(captured, f).view(torch.uint8), getattr(eager, f).view(torch.uint8)), f


# ---- end to end: a model's field, its parts, their twists, their joints ------------------------------------------------------------
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


def test_cloud_joints_end_to_end(model, dev):
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_components, cloud_joints, cloud_twists, dominant_joint,
                                                        extract_field)
    grid = FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), (17, 13, 11))
    enc = _encoding(2, dev)
    head, _ = model.compute_density(grid.points(device=dev)[None].expand(2, -1, 3).contiguous(), enc)
    dense = head.density.reshape(-1).double().cpu()
    cloud = extract_field(model, enc, grid, float(torch.quantile(dense, 0.6)))
    assert cloud.index.shape[0] > 100
    labels, sizes, _ = cloud_components(cloud, keys=dominant_joint(cloud.jacobian))
    tw = cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=2, max_parts=64)
    joints = cloud_joints(cloud, labels, tw)
    given = cloud_joints(cloud, labels, tw, batch=2)
    for f in R.OUTPUTS:
        assert torch.equal(getattr(joints, f).view(torch.uint8), getattr(given, f).view(torch.uint8)), f
    # the restatement, fed the same tensors
    cpu = lambda t: t.cpu().numpy()   # noqa: E731
    ref = R.joints(grid.dims, grid.origin, grid.step, 2, cpu(cloud.index), cpu(labels), cpu(tw.labels), cpu(tw.status),
                   cpu(tw.centroid), cpu(tw.omega), cpu(tw.velocity), parts_count=int(tw.count.item()), count=int(cloud.count.item()))
    _same_bytes(joints, ref)
    count = int(joints.count.item())
    print(f"{cloud.index.shape[0]} rows, {int(tw.count.item())} parts of at least 2 nodes, {count} joints among the first 64")
    assert count >= 1
    parent, joint_of = joints.parents()
    stored = min(count, 256)
    hung = parent >= 0
    assert tuple(parent.shape) == (64,) and int(hung.sum()) <= stored and (joint_of[hung] < stored).all()
    a, b = joints.part_a.cpu()[joint_of[hung]].long(), joints.part_b.cpu()[joint_of[hung]].long()
    slot = torch.arange(64)[hung]
    assert (((a == slot) & (b == parent[hung])) | ((b == slot) & (a == parent[hung]))).all()   # a slot hangs on its joint's other end
