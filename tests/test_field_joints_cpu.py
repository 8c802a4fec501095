"""Host-side tests of the joints between parts (field_volume.part_joints / cloud_joints / FieldJoints; njf_field_joints;
DESIGN.md section 16): the numpy restatement (tests/field_joints_restatement.py) against its own node-pair loop, the planted
3-link chain, ``screw()`` / ``drive()`` / ``parents()`` on CPU tensors, every argument check -- raised before any device work:
there is no GPU here -- and the C ABI's symbol and return codes."""
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import field_joints_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 29


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


@pytest.fixture(scope="module")
def chain():
    return R.chain()


@pytest.fixture(scope="module")
def blocks():
    return R.blocks()


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", (6, 14))
def test_the_vectorised_restatement_equals_its_node_pair_loop(chain, blocks, connectivity):
    for scene in (chain, blocks):
        ref = R.run(scene, connectivity=connectivity)
        loop = R.run(scene, connectivity=connectivity, table=R.tables_loop)
        for t, u in zip(ref["table"], loop["table"]):
            assert np.array_equal(t, u)
        for f in R.OUTPUTS:
            assert ref[f].tobytes() == loop[f].tobytes(), f
        assert ref["count"][0] > 0 and not np.tril(ref["table"][0]).any()          # only lo < hi is ever filled


def test_the_blocks_scene_is_what_the_issue_describes(blocks):
    dims, nodes = blocks["dims"], R.BLOCK_DIMS[0] * R.BLOCK_DIMS[1] * R.BLOCK_DIMS[2]
    count, index, labels, parts = blocks["count"], blocks["index"], blocks["labels"], blocks["parts"]
    listed = index[1:count - 1]
    assert (np.diff(listed.astype(np.int64)) > 0).all() and index[0] < 0 and index[count - 1] >= 2 * nodes
    assert index.shape[0] > count and (np.diff(parts) > 0).all()
    assert (labels[:count] == -1).sum() == 30 and blocks["outside_label"] not in parts and (labels == blocks["outside_label"]).any()
    assert (labels[:count] == blocks["single"]).sum() == 1 and blocks["single"] in parts
    assert blocks["status"][3] == R.TRANSLATION
    # the part that ends on the last node of element 0 and the one that starts on node 0 of element 1 are listed, and not joined
    slot = R.slots(labels, parts, None, count)
    last, first = slot[index == nodes - 1][0], slot[index == nodes][0]
    assert last >= 0 and first >= 0 and last != first
    for connectivity in (6, 14):
        ref = R.run(blocks, connectivity=connectivity)
        contacts = ref["table"][0]
        assert contacts[min(last, first), max(last, first)] == 0
        element = np.array([p // nodes for p in parts])
        lo, hi = np.nonzero(contacts)
        assert (element[lo] == element[hi]).all()                                   # nothing crosses batch elements
        # every part touches only parts whose blocks are its neighbours: no wrap from the end of a row or plane to the next
        assert ref["count"][0] == np.count_nonzero(contacts) and ref["count"][0] < 256
        # rows past the count are never read: reading them would add contacts
        assert R.run(blocks, connectivity=connectivity, count=None)["table"][0].sum() > contacts.sum()
    # the wrap itself: node (ix, iy, nz - 1) and (ix, iy + 1, 0) are one apart in linear index and belong to different parts
    a, b = slot[index == dims[2] - 1][0], slot[index == dims[2]][0]
    assert a >= 0 and b >= 0 and a != b and R.run(blocks)["table"][0][min(a, b), max(a, b)] == 0


def test_the_planted_chain(chain):
    ref = R.run(chain)
    assert ref["count"][0] == 2
    assert ref["part_a"][:2].tolist() == [0, 1] and ref["part_b"][:2].tolist() == [1, 2]
    assert ref["contacts"][:2].tolist() == [R.CHAIN_FACE_PAIRS] * 2                  # the face's node pairs at connectivity 6
    o, s = np.asarray(R.ORIGIN, np.float32).astype(np.float64), np.asarray(R.STEP, np.float32).astype(np.float64)
    for j, centre in enumerate(R.CHAIN_FACE_CENTRES):
        assert np.array_equal(ref["anchor"][j], o + s * np.array(centre))           # the face centres, exactly
    assert (ref["part_a"][2:] == -1).all() and (ref["part_b"][2:] == -1).all()
    for f in ("contacts", "status", "anchor", "omega", "velocity"):
        assert not ref[f][2:].any(), f
    joints = R.field_joints(chain, ref, R.field_twists(chain))
    assert joints.drive()[:2].tolist() == [0, 1]
    # the hinge channels leave the anchor at rest: |v| at rounding level of |omega| * (the distance to the centroid)
    for j, a in ((0, 0), (1, 1)):
        w = np.linalg.norm(ref["omega"][j, a])
        assert w > 0.5 and np.linalg.norm(ref["velocity"][j, a]) <= 1e-14 * w
    assert np.abs(ref["velocity"][1, 0]).max() <= 1e-14 and not ref["omega"][1, 0].any()   # channel 0 carries link 2 with link 1
    assert not ref["omega"][:, 2].any() and not ref["velocity"][:, 2].any()
    direction, point, pitch = joints.screw()
    assert torch.allclose(direction[0, 0], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    assert torch.allclose(direction[1, 1], torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64))
    assert torch.allclose(point[0, 0], joints.anchor[0], atol=1e-13) and torch.allclose(point[1, 1], joints.anchor[1], atol=1e-13)
    assert abs(float(pitch[0, 0])) < 1e-13 and abs(float(pitch[1, 1])) < 1e-13
    parent, joint_of = joints.parents()
    assert parent.tolist() == [-1, 0, 1] and joint_of.tolist() == [-1, 0, 1]        # the chain, hung on the base
    parent, joint_of = joints.parents(root=2)
    assert parent.tolist() == [1, 2, -1] and joint_of.tolist() == [0, 1, -1]
    # at connectivity 14 the diagonals across the faces count too: the base is a node wider than link 1 on every side, so all
    # four directions with dx = 1 find 16 pairs; the links have equal cross-sections, which leaves 16 + 12 + 12 + 9
    wide = R.run(chain, connectivity=14)
    assert wide["contacts"][:2].tolist() == [4 * 16, 16 + 12 + 12 + 9] and wide["count"][0] == 2
    assert np.array_equal(wide["anchor"][:2, 0], ref["anchor"][:2, 0])              # the faces' x: every pair has the same


# ---- FieldJoints methods on CPU tensors ---------------------------------------------------------------------------------------------
def _joints(part_a, part_b, contacts, omega, velocity, anchor=None, k=None, step=(0.5, 0.25, 0.125), twists=None, count=None):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldJoints
    j = len(part_a)
    k = max(part_b) + 1 if k is None else k
    f64 = torch.float64
    omega, velocity = torch.as_tensor(omega, dtype=f64).reshape(j, -1, 3), torch.as_tensor(velocity, dtype=f64).reshape(j, -1, 3)
    return FieldJoints(grid=FieldGrid((0.0, 0.0, 0.0), step, (4, 4, 4)), labels=torch.arange(k, dtype=torch.int32) * 10,
                       part_a=torch.tensor(part_a, dtype=torch.int32), part_b=torch.tensor(part_b, dtype=torch.int32),
                       contacts=torch.tensor(contacts, dtype=torch.int64), status=torch.zeros(j, dtype=torch.int32),
                       count=torch.tensor([j if count is None else count], dtype=torch.int32),
                       anchor=torch.zeros(j, 3, dtype=f64) if anchor is None else torch.as_tensor(anchor, dtype=f64),
                       omega=omega, velocity=velocity, twists=twists)


def test_screw_of_a_rotation_a_prismatic_joint_and_a_zero_twist():
    axis = torch.tensor([2.0, 1.0, 2.0], dtype=torch.float64) / 3.0
    anchor = torch.tensor([[0.3, -0.1, 0.7]], dtype=torch.float64)
    on_axis = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    rate, pitch = 0.4, 0.25
    v_rot = torch.linalg.cross(rate * axis, anchor[0] - on_axis)
    zero = torch.zeros(3, dtype=torch.float64)
    slide = torch.tensor([0.0, 3.0, 4.0], dtype=torch.float64)
    omega = torch.stack([rate * axis, zero, rate * axis, zero])
    velocity = torch.stack([v_rot, slide, v_rot + pitch * rate * axis, zero])
    joints = _joints([0], [1], [5], omega, velocity, anchor=anchor)
    direction, point, got = joints.screw()
    foot = on_axis + torch.dot(anchor[0] - on_axis, axis) * axis                   # the point of the hinge line nearest the anchor
    for a in (0, 2):
        assert torch.allclose(direction[0, a], axis, atol=1e-15) and torch.allclose(point[0, a], foot, atol=1e-14)
    assert abs(float(got[0, 0])) < 1e-15 and abs(float(got[0, 2]) - pitch) < 1e-15
    assert torch.allclose(direction[0, 1], slide / 5.0) and torch.equal(point[0, 1], anchor[0]) and math.isinf(float(got[0, 1]))
    assert not direction[0, 3].any() and torch.equal(point[0, 3], anchor[0])
    assert not any(torch.isnan(t).any() for t in (direction, point))
    # the prismatic test is |omega| * (the largest grid step) <= eps * |v|
    tiny = _joints([0], [1], [5], omega[:1] * 1e-9, slide[None], anchor=anchor)
    assert math.isinf(float(tiny.screw()[2][0, 0]))                                 # 0.4e-9 * 0.5 <= 1e-9 * 5
    assert math.isfinite(float(tiny.screw(eps=1e-12)[2][0, 0]))
    fine = _joints([0], [1], [5], omega[:1] * 1e-9, slide[None], anchor=anchor, step=(50.0, 1.0, 1.0))
    assert math.isfinite(float(fine.screw()[2][0, 0]))                              # 0.4e-9 * 50 > 1e-9 * 5


def test_drive_picks_the_strongest_channel_and_the_lowest_on_ties():
    omega = [[[0, 0, 1.0], [0, 0, 0], [0, 0, 0]], [[0, 0, 0], [2.0, 0, 0], [2.0, 0, 0]], [[0, 0, 0]] * 3]
    velocity = [[[0, 0, 0], [0.4, 0, 0], [0, 0, 0]], [[0, 0, 0]] * 3, [[0, 0, 0]] * 3]
    joints = _joints([0, 0, -1], [1, 2, -1], [3, 3, 0], omega, velocity, k=3, count=2)
    assert joints.drive().dtype == torch.int64
    assert joints.drive().tolist() == [0, 1, 0]            # 1 * 0.5^2 > 0.4^2; a tie goes to the lowest channel; an unused row
    assert joints.drive(length=0.25).tolist() == [1, 1, 0]  # 1 * 0.25^2 < 0.4^2


def test_parents_of_a_forest_of_two_bodies_with_ties():
    from neural_jacobian_field_amd.field_volume import FieldTwists
    # body one: slots 0-1-2-3 in a ring with a chord; body two: slots 4-5; slot 6 touches nothing; slot 7 is unused
    part_a, part_b, contacts = [0, 0, 0, 1, 2, 4], [1, 2, 3, 2, 3, 5], [5, 9, 5, 9, 5, 1]
    k, j = 8, len(part_a)
    z = torch.zeros(j, 1, 3)
    f64 = torch.float64
    energy = torch.tensor([[3.0], [0.5], [4.0], [0.0], [2.0], [1.0], [0.0], [0.0]], dtype=f64)
    weight = torch.tensor([1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 0.0], dtype=f64)
    status = torch.tensor([0, 0, 0, 2, 0, 0, 0, 0], dtype=torch.int32)          # slot 3 is still, but translation-only: no base
    labels = torch.tensor([0, 10, 20, 30, 40, 50, 60, -1], dtype=torch.int32)
    twists = FieldTwists(labels=labels, count=torch.tensor([7], dtype=torch.int32), nodes=weight.to(torch.int32), status=status,
                         weight=weight, centroid=torch.zeros(k, 3, dtype=f64), omega=torch.zeros(k, 1, 3, dtype=f64),
                         velocity=torch.zeros(k, 1, 3, dtype=f64), energy=energy, residual=torch.zeros(k, 1, dtype=f64),
                         Q=torch.zeros(k, 6, dtype=f64), P=torch.zeros(k, 1, 3, dtype=f64), L=torch.zeros(k, 1, 3, dtype=f64),
                         row_residual=torch.zeros(0))
    joints = dataclasses.replace(_joints(part_a, part_b, contacts, z, z, k=k, twists=twists), labels=labels)
    parent, joint_of = joints.parents()
    # the forest keeps (0,2) and (1,2) -- 9 contacts each --, then of the three ties at 5 the smallest pair that joins: (0,3);
    # (0,1) and (2,3) would close rings.  Body one hangs on slot 1 (0.5 / 1, the smallest among status 0), body two on slot 5.
    assert parent.tolist() == [2, -1, 1, 0, 5, -1, -1, -1]
    assert joint_of.tolist() == [1, -1, 3, 2, 5, -1, -1, -1]
    parent, joint_of = joints.parents(root=3)
    assert parent.tolist() == [3, 2, 0, -1, 5, -1, -1, -1] and joint_of.tolist() == [2, 3, 1, -1, 5, -1, -1, -1]
    # rows past the count are not joints; without twists the smallest slot of a body is its root
    fewer = dataclasses.replace(joints, count=torch.tensor([5], dtype=torch.int32), twists=None)
    parent, _ = fewer.parents()
    assert parent.tolist() == [-1, 2, 0, 0, -1, -1, -1, -1]
    for bad in (-1, 8, 1.0, True):
        with pytest.raises(ValueError, match="root must be a slot"):
            joints.parents(root=bad)
    with pytest.raises(ValueError, match="slot 7 is unused"):
        joints.parents(root=7)


# ---- argument errors ------------------------------------------------------------------------------------------------------------------
def test_part_joints_checks_its_arguments_before_any_gpu_work(chain):
    from neural_jacobian_field_amd.field_volume import FieldGrid, part_joints
    grid = FieldGrid(chain["origin"], chain["step"], chain["dims"])
    index, labels = torch.from_numpy(chain["index"]), torch.from_numpy(chain["labels"])
    tw = R.field_twists(chain)
    n = index.shape[0]
    good = dict(batch=2)
    for bad in (26, 0, True, None):
        with pytest.raises(ValueError, match="connectivity must be 6 or 14"):
            part_joints(grid, index, labels, tw, connectivity=bad, **good)
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="min_contacts must be"):
            part_joints(grid, index, labels, tw, min_contacts=bad, **good)
    for bad in (0, 4097, 2.0, True, None):
        with pytest.raises(ValueError, match="max_joints must be"):
            part_joints(grid, index, labels, tw, max_joints=bad, **good)
    for bad in (0, -2, 1.0, True, None, 2 ** 31 // grid.num_nodes + 1):
        with pytest.raises(ValueError, match="batch must be"):
            part_joints(grid, index, labels, tw, batch=bad)
    for bad in (index.long(), index.reshape(1, n), index.float(), None):
        with pytest.raises(ValueError, match="index must be int32"):
            part_joints(grid, bad, labels, tw, **good)
    for bad in (labels.long(), labels[:-1], labels.reshape(n, 1), None):
        with pytest.raises(ValueError, match="labels must be int32"):
            part_joints(grid, index, bad, tw, **good)
    with pytest.raises(ValueError, match="twists must be a FieldTwists"):
        part_joints(grid, index, labels, None, **good)
    with pytest.raises(ValueError, match="twists.labels must be int32"):
        part_joints(grid, index, labels, dataclasses.replace(tw, labels=tw.labels.long()), **good)
    for k in (0, 257):
        many = dataclasses.replace(tw, labels=torch.zeros(k, dtype=torch.int32))
        with pytest.raises(ValueError, match="1 to 256 parts"):
            part_joints(grid, index, labels, many, **good)
    for bad in (tw.omega.float(), tw.omega[:2], tw.omega.reshape(3, 9), tw.omega[:, :, :2]):
        with pytest.raises(ValueError, match="twists.omega must be float64"):
            part_joints(grid, index, labels, dataclasses.replace(tw, omega=bad), **good)
    for a in (0, 11):
        with pytest.raises(ValueError, match="1 to 10 command channels"):
            part_joints(grid, index, labels, dataclasses.replace(tw, omega=torch.zeros(3, a, 3, dtype=torch.float64)), **good)
    for field, bad in (("velocity", tw.velocity[:, :2]), ("velocity", tw.velocity.float()), ("centroid", tw.centroid[:2]),
                       ("centroid", tw.centroid.float()), ("status", tw.status.long()), ("status", tw.status[:1])):
        with pytest.raises(ValueError, match=f"twists.{field} must be"):
            part_joints(grid, index, labels, dataclasses.replace(tw, **{field: bad}), **good)
    for bad in (3, torch.ones(2, dtype=torch.int32), torch.ones(1)):
        with pytest.raises(ValueError, match="count must be one int32"):
            part_joints(grid, index, labels, tw, count=bad, **good)
        with pytest.raises(ValueError, match="twists.count must be one int32"):
            part_joints(grid, index, labels, dataclasses.replace(tw, count=bad), **good)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="must live on the device"):
            part_joints(grid, index.cuda(), labels, tw, **good)
    with pytest.raises(ValueError, match="no CPU path"):
        part_joints(grid, index, labels, tw, count=torch.tensor([n], dtype=torch.int32), **good)


def test_cloud_joints_checks_its_arguments_before_any_gpu_work(chain):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud, cloud_joints
    grid = FieldGrid(chain["origin"], chain["step"], chain["dims"])
    index, labels = torch.from_numpy(chain["index"]), torch.from_numpy(chain["labels"])
    n = index.shape[0]
    cloud = FieldPointCloud(grid=grid, index=index, xyz=torch.zeros(n, 3), density=torch.ones(n), color=None, jacobian=None,
                            count=torch.tensor([n], dtype=torch.int32))
    tw = R.field_twists(chain)
    with pytest.raises(ValueError, match="cloud_joints: connectivity must be 6 or 14"):
        cloud_joints(cloud, labels, tw, connectivity=8)
    with pytest.raises(ValueError, match="cloud_joints: labels must be int32"):
        cloud_joints(cloud, labels[:-1], tw)
    with pytest.raises(ValueError, match="cloud_joints: max_joints must be"):
        cloud_joints(cloud, labels, tw, max_joints=0)
    with pytest.raises(ValueError, match="cloud_joints: batch must be"):
        cloud_joints(cloud, labels, tw, batch=0)
    for batch in (None, 2):                                 # with and without the batch: refused before anything is read
        with pytest.raises(ValueError, match="cloud_joints: .*no CPU path"):
            cloud_joints(cloud, labels, tw, batch=batch)


def test_the_signatures():
    from neural_jacobian_field_amd import field_volume
    params = inspect.signature(field_volume.part_joints).parameters
    assert list(params) == ["grid", "index", "labels", "twists", "batch", "count", "connectivity", "min_contacts", "max_joints"]
    defaults = dict(count=None, connectivity=6, min_contacts=1, max_joints=256)
    assert {k: params[k].default for k in defaults} == defaults and params["batch"].default is inspect.Parameter.empty
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("batch", *defaults))
    params = inspect.signature(field_volume.cloud_joints).parameters
    assert list(params) == ["cloud", "labels", "twists", "batch", "connectivity", "min_contacts", "max_joints"]
    defaults = dict(batch=None, connectivity=6, min_contacts=1, max_joints=256)
    assert {k: params[k].default for k in defaults} == defaults
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in defaults)
    fields = list(field_volume.FieldJoints.__dataclass_fields__)
    assert set(R.OUTPUTS) | {"labels"} <= set(fields)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "njf_field_joints" in declared and "njf_field_joints" in hip.EXPORTED_SYMBOLS and hasattr(lib, "njf_field_joints")
    params = re.search(r"njf_field_joints\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_joints.argtypes) == ARGUMENTS
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_JOINTS_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_JOINTS_MAX"] == hip.FIELD_JOINTS_MAX == 4096
    assert defines["NJF_FIELD_JOINTS_ALL"] == hip.FIELD_JOINTS_ALL == sum(hip.FIELD_JOINTS_PHASES)
    assert defines["NJF_FIELD_JOINTS_PER_LANE"] == hip.FIELD_JOINTS_PER_LANE == hip.FIELD_JOINTS_ALL + 1
    assert [defines[f"NJF_FIELD_JOINTS_{n.upper()}"] for n in hip.FIELD_JOINTS_PHASE_NAMES] == list(hip.FIELD_JOINTS_PHASES)
    # the workspace: 4 K^2 table words and the int32 volume, two nodes per 64-bit word
    assert "NJF_FIELD_JOINTS_WORKSPACE(total, K)" in header
    assert hip.field_joints_workspace(1001, 3) == 36 + 501 and hip.field_joints_workspace(0, 256) == 4 * 65536


def test_the_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    import ctypes as C
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("grid", "batch", "indices", "labels", "count", "n", "parts", "parts_count", "num_parts", "part_status", "centroid",
             "omega", "velocity", "action_dim", "connectivity", "min_contacts", "max_joints", "part_a", "part_b", "contacts",
             "status", "out_count", "anchor", "out_omega", "out_velocity", "workspace", "workspace_words", "phases")
    assert len(names) + 1 == ARGUMENTS
    grid = hip.make_field_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (10, 10, 10))
    need = hip.field_joints_workspace(2000, 4)

    def call(**kw):
        args = {k: P for k in names}
        args.update(grid=C.byref(grid), batch=2, n=500, num_parts=4, action_dim=8, connectivity=6, min_contacts=1, max_joints=16,
                    workspace_words=need, phases=31)
        args.update(kw)
        return lib.njf_field_joints(*[args[k] for k in names], None)

    for bad in (0, 8, 26, -6):
        assert call(connectivity=bad) == E_VALUE
    for bad in (0, -3, 257):
        assert call(num_parts=bad) == E_VALUE
    for bad in (0, -1, 11):
        assert call(action_dim=bad) == E_VALUE
    for bad in (0, -1, 4097):
        assert call(max_joints=bad) == E_VALUE
    for bad in (0, -5):
        assert call(min_contacts=bad) == E_VALUE
    for bad in (0, -1, 64, 128):
        assert call(phases=bad) == E_VALUE
    assert call(n=-1) == E_SHAPE
    assert call(batch=0) == E_SHAPE
    assert call(workspace_words=need - 1) == E_SHAPE                            # the workspace is too small
    big = hip.make_field_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1024, 1024, 1024))
    assert call(grid=C.byref(big), batch=2, workspace_words=2 ** 62) == E_SHAPE  # B*N = 2^31
    for key in names:
        if key in ("count", "parts_count", "batch", "n", "num_parts", "action_dim", "connectivity", "min_contacts", "max_joints",
                   "workspace_words", "phases"):
            continue                                                            # (optional pointers, integers)
        assert call(**{key: None}) == E_NULL, key
    # the rows may be absent when there are none, the outputs may not
    assert call(n=0, indices=None, labels=None, part_a=None) == E_NULL
