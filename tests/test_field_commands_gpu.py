"""GPU tests of inverse kinematics on the part tree (field_volume.solve_commands / cloud_commands; njf_field_commands; DESIGN.md
section 18) against the numpy restatement of its semantics (tests/field_commands_restatement.py).

Moments: per entry ``|dev - ref| <= (n_p + 3) 2^-53 sum |terms|`` against the exactly rounded sums, the worst case of any summation
order.  Solver honesty: the device's cost, initial cost and gradient against the restatement's sums over the ROWS at the
device's own commands (the iterate is fp32, so the restatement evaluates the very same point): ``|d cost| <= 1e-13 E / W`` and
``|d g|_inf <= 1e-12 max(1, |g_0|_inf)``, ``E = sum w (|x~|^2 + |y~|^2)``, ``g_0`` the gradient at the start.  Solver quality: five
more iterations of the restatement from the device's commands lower L by at most ``1e-9 L + 2e-13 E / W``.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_commands_restatement as F
import field_joints_restatement as J
import field_pose_restatement as R

pytestmark = pytest.mark.gpu

IMG = 64
COST_TOL = 2e-13
OUTPUTS = ("commands", "cost", "initial_cost", "weight", "steps", "gradient", "status", "part_status", "depth", "moments")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _one(dev, v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=dev)


def _np(t):
    return t.cpu().numpy()


def _grid(scene):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid(scene["origin"], scene["step"], scene["dims"])


class Scene:
    """A scene of the restatements on the device: twists, joints and tree (``part_joints`` of the device, or given), the rows,
    and the same as numpy dicts for the restatement."""

    def __init__(self, dev, scene, tree=True, given=None):
        from neural_jacobian_field_amd.field_volume import part_joints
        self.dev, self.scene = dev, scene
        self.count = scene.get("count")
        if given is None:
            self.tw = J.field_twists(scene, dev)
            self.xyz = J.node_coordinates(scene["dims"], scene["index"]).astype(np.float32)
            self.labels = scene["labels"]
            self.joints = self.tree = None
            if tree:
                index, labels = torch.from_numpy(scene["index"]).to(dev), torch.from_numpy(scene["labels"]).to(dev)
                self.joints = part_joints(_grid(scene), index, labels, self.tw, batch=scene["batch"], count=_one(dev, self.count))
                self.tree = self.joints.tree()
        else:
            self.tw, self.joints, self.tree, self.xyz, self.labels = given
        self.parts = _np(self.tw.labels)
        self.twists = dict(status=_np(self.tw.status), count=int(self.tw.count.item()), centroid=_np(self.tw.centroid),
                           omega=_np(self.tw.omega), velocity=_np(self.tw.velocity))
        self.refresh()

    def refresh(self):
        j = self.joints
        self.jd = None if j is None else dict(part_a=_np(j.part_a), part_b=_np(j.part_b), count=int(j.count.item()),
                                              anchor=_np(j.anchor), omega=_np(j.omega), velocity=_np(j.velocity))
        self.td = None if self.tree is None else tuple(_np(t) for t in self.tree)

    def targets(self, commands):
        return F.posed_targets(self.twists, np.asarray(commands, np.float32), self.xyz, self.labels, self.parts, self.jd, self.td,
                               count=self.count)

    def solve(self, targets, weights=None, **kw):
        from neural_jacobian_field_amd.field_volume import solve_commands
        t = lambda v: None if v is None else (torch.from_numpy(np.ascontiguousarray(v)).to(self.dev) if isinstance(v, np.ndarray) else v)   # noqa: E731
        kw = {k: t(v) for k, v in kw.items()}
        return solve_commands(self.tw, t(self.xyz), t(self.labels), t(targets), joints=self.joints, tree=self.tree, weights=t(weights),
                              count=_one(self.dev, self.count), **kw)

    def restatement(self, targets, **kw):
        return F.solve(self.twists, self.xyz, self.labels, targets, self.parts, self.jd, self.td, count=self.count, **kw)


def _check_moments(s, fit, targets, weights=None):
    """(a): the device's moments against the exactly rounded sums; returns ``(moments, E, W)`` of the restatement."""
    status, depth = F.pose_status(s.twists, s.jd, s.td)
    assert np.array_equal(_np(fit.part_status), status) and np.array_equal(_np(fit.depth), depth)
    ref, bound = F.moments(s.xyz, s.labels, targets, s.parts, s.twists["count"], status, s.twists["centroid"], weights, s.count)
    got = _np(fit.moments)
    assert got.shape == ref.shape and fit.moments.dtype == torch.float64
    err = np.abs(got - ref)
    ratio = (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0
    print(f"moments: worst ratio to the bound {ratio:.4f} over {int((bound > 0).sum())} entries; {int((ref[..., 0] > 0).sum())} (m, p) with rows")
    assert (err <= bound).all()                                  # (an entry without a term has bound 0: it must be exactly 0)
    energy, total = F.energy(ref)
    return ref, energy, total


def _check_honesty(s, fit, targets, weights=None, init=None, lower=None, upper=None, reg=0.0, energy=None, total=None, problems=None):
    """(b): cost, initial cost and gradient against the restatement's sums over the rows at the device's own commands."""
    m, a_dim = targets.shape[0], s.twists["omega"].shape[1]
    status = _np(fit.part_status)
    slot, w = F.counted(s.xyz, s.labels, targets, s.parts, s.twists["count"], status, weights, s.count)
    commands = _np(fit.commands)
    assert commands.dtype == np.float32 and commands.shape == (m, a_dim)
    box = lambda v, fill: np.broadcast_to(np.float32(fill if v is None else v), (m, a_dim))   # noqa: E731
    start = np.minimum(np.maximum(box(init, 0.0), box(lower, -np.inf)), box(upper, np.inf)).astype(np.float32)
    worst = [0.0, 0.0]
    for i in range(m) if problems is None else problems:
        if _np(fit.status)[i]:
            continue
        first = F.evaluate_rows(s.xyz, slot, w[i], targets[i], F.chain(s.twists, start[i], s.jd, s.td))
        last = F.evaluate_rows(s.xyz, slot, w[i], targets[i], F.chain(s.twists, commands[i], s.jd, s.td))
        scale = energy[i] / total[i]
        g0 = np.abs(first[1] + reg / a_dim * start[i].astype(np.float64)).max()
        g = last[1] + reg / a_dim * commands[i].astype(np.float64)
        dc = max(abs(_np(fit.cost)[i] - max(last[0], 0.0)), abs(_np(fit.initial_cost)[i] - max(first[0], 0.0))) / (1e-13 * scale)
        dg = np.abs(_np(fit.gradient)[i] - g).max() / (1e-12 * max(1.0, g0))
        worst = [max(worst[0], dc), max(worst[1], dg)]
        assert abs(_np(fit.weight)[i] - last[3]) <= 1e-12 * last[3]
    print(f"honesty: worst ratio to the bound, cost {worst[0]:.4f}, gradient {worst[1]:.4f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def _check_quality(s, fit, targets, energy, total, problems, **kw):
    """(c): five more iterations of the restatement from the device's commands lower L by at most 1e-9 L + 2e-13 E / W."""
    more = s.restatement(targets, init=_np(fit.commands), iterations=5, **kw)
    a_dim = s.twists["omega"].shape[1]
    reg = kw.get("reg", 0.0)
    for i in problems:
        u0, u1 = _np(fit.commands)[i].astype(np.float64), more["commands"][i].astype(np.float64)
        before = more["initial_cost"][i] + reg / a_dim * (u0 @ u0)
        after = more["cost"][i] + reg / a_dim * (u1 @ u1)
        print(f"quality: problem {i}: L {before:.3e} -> {after:.3e} in {more['steps'][i]} more steps")
        assert before - after <= 1e-9 * before + COST_TOL * energy[i] / total[i]


# ---- the planted chain ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(dev):
    return Scene(dev, J.chain())


def _planted(count, seed=4):
    rng = np.random.default_rng(seed)
    u = np.stack([rng.uniform(-1, 1, count) * 0.98 / 0.7, rng.uniform(-1, 1, count) * 0.98 / 1.3, np.zeros(count)], axis=1)
    return u.astype(np.float32)


@pytest.mark.parametrize("m", (1, 3, 70))
def test_the_planted_chain(dev, chain, m):
    planted = _planted(m)
    targets = chain.targets(planted)
    start = np.zeros((m, 3), np.float32)
    start[:, 2] = np.linspace(-1.0, 1.0, m, dtype=np.float32)
    fit = chain.solve(targets, init=start)
    for f, shape, dtype in (("commands", (m, 3), torch.float32), ("cost", (m,), torch.float64), ("initial_cost", (m,), torch.float64),
                            ("weight", (m,), torch.float64), ("steps", (m,), torch.int32), ("gradient", (m, 3), torch.float64),
                            ("status", (m,), torch.int32), ("part_status", (3,), torch.int32), ("depth", (3,), torch.int32),
                            ("moments", (m, 3, 23), torch.float64)):
        t = getattr(fit, f)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cuda", f
    _, energy, total = _check_moments(chain, fit, targets)
    _check_honesty(chain, fit, targets, init=start, energy=energy, total=total)
    assert not fit.status.any() and fit.depth.tolist() == [0, 1, 2]
    ratio = _np(fit.cost) / (COST_TOL * energy / total)
    print(f"planted chain: accepted steps <= {int(fit.steps.max())}, worst cost / bound {ratio.max():.4f}")
    assert (ratio <= 1.0).all()
    assert _np(fit.commands)[:, 2].tobytes() == start[:, 2].tobytes()          # channel 2 moves nothing: bitwise its start
    assert np.abs(_np(fit.commands)[:, :2] - planted[:, :2]).max() <= 1e-6
    assert torch.equal(fit.rms(), fit.cost.sqrt())
    # (the restatement is slow in numpy: three problems are held to the quality bound, spread over the tiles of 16 problems)
    _check_quality(chain, fit, targets, energy, total, sorted({0, 17 % m, m - 1}))
    # the pose at the returned commands is the pose whose cost is reported
    from neural_jacobian_field_amd.field_volume import part_poses
    pose = part_poses(chain.tw, fit.commands, joints=chain.joints, tree=chain.tree)
    assert torch.equal(pose.status, fit.part_status) and torch.equal(pose.depth, fit.depth)


def test_one_iteration_and_none(dev, chain):
    targets = chain.targets(_planted(4, seed=8))
    one, ref = chain.solve(targets, iterations=1), chain.restatement(targets, iterations=1)
    got, want = _np(one.commands), ref["commands"]
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all() and _np(one.steps).tolist() == ref["steps"].tolist() == [1] * 4
    start = np.float32([[3.0, -0.2, 0.1]] * 4)
    none = chain.solve(targets, iterations=0, init=start, lower=-1.0, upper=torch.tensor([1.0, 2.0, 3.0], device=dev))
    assert _np(none.commands).tolist() == [[1.0, np.float32(-0.2), np.float32(0.1)]] * 4 and not none.steps.any()
    assert torch.equal(none.cost, none.initial_cost)
    _, energy, total = _check_moments(chain, none, targets)
    _check_honesty(chain, none, targets, init=start, lower=-1.0, upper=np.float32([1.0, 2.0, 3.0]), energy=energy, total=total)


def test_bounds_noise_and_the_regulariser(dev, chain):
    planted = np.float32([[0.9, -0.7, 0.0], [0.5, 0.3, 0.0], [-0.8, 0.6, 0.0]])
    clean = chain.targets(planted)
    fit = chain.solve(clean, lower=-0.5, upper=0.5)
    assert _np(fit.commands)[0].tolist() == [0.5, -0.5, 0.0]
    g = _np(fit.gradient)[0]
    assert g[0] < 0.0 and g[1] > 0.0 and g[2] == 0.0
    _, energy, total = _check_moments(chain, fit, clean)
    _check_honesty(chain, fit, clean, lower=-0.5, upper=0.5, energy=energy, total=total)
    _check_quality(chain, fit, clean, energy, total, range(3), lower=-0.5, upper=0.5)
    rng = np.random.default_rng(3)
    for noise in (0.01, 0.05):
        noisy = (clean + noise * rng.normal(size=clean.shape)).astype(np.float32)
        for reg in (0.0, 1e-3):
            fit = chain.solve(noisy, reg=reg)
            _, energy, total = _check_moments(chain, fit, noisy)
            _check_honesty(chain, fit, noisy, reg=reg, energy=energy, total=total)
            _check_quality(chain, fit, noisy, energy, total, range(3), reg=reg)
            assert (_np(fit.cost) <= _np(fit.initial_cost)).all()
    free, held = chain.solve(clean), chain.solve(clean, reg=1e-3)
    assert (torch.linalg.vector_norm(held.commands, dim=1) < torch.linalg.vector_norm(free.commands, dim=1)).all()


def test_handles_and_empty_problems(dev, chain):
    planted = np.float32([[0.6, -0.4, 0.0]] * 4)
    full = chain.targets(planted)
    tip = np.flatnonzero(chain.labels == chain.parts[2])
    targets = np.full_like(full, np.nan)
    targets[0, tip[[0, 5, 40, 63]]] = full[0, tip[[0, 5, 40, 63]]]
    targets[1, tip[17]] = full[1, tip[17]]
    targets[3, tip[3], :2] = full[3, tip[3], :2]                      # one NaN coordinate: the row is not counted
    start = np.float32([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.2, -3.0, 1.0], [0.1, 0.1, 0.1]])
    fit = chain.solve(targets, init=start, lower=-1.0, upper=1.0)
    assert fit.status.tolist() == [0, 0, F.NO_ROWS, F.NO_ROWS] and fit.weight.tolist() == [4.0, 1.0, 0.0, 0.0]
    assert _np(fit.commands)[2].tolist() == [np.float32(0.2), -1.0, 1.0] and _np(fit.commands)[3].tobytes() == start[3].tobytes()
    assert not fit.cost[2:].any() and not fit.steps[2:].any() and not fit.moments[2:].any() and not fit.gradient[2:].any()
    _, energy, total = _check_moments(chain, fit, targets)
    _check_honesty(chain, fit, targets, init=start, lower=-1.0, upper=1.0, energy=energy, total=total)
    assert np.abs(_np(fit.commands)[:2] - planted[:2]).max() <= 1e-5       # four handles, and one: three equations for two channels
    assert (_np(fit.cost)[:2] <= COST_TOL * energy[:2] / total[:2]).all()
    not_finite = chain.solve(full[:1], init=np.float32([[np.inf, 0.0, 0.0]]))
    assert not_finite.status.tolist() == [F.NOT_FINITE] and not_finite.steps.tolist() == [0]
    assert _np(not_finite.commands)[0].tolist() == [np.inf, 0.0, 0.0]


# ---- 53 parts and an unused slot: every kind of row, weights of both shapes ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def blocks(dev):
    scene = J.blocks()
    assert scene["parts"].shape[0] == 54 and scene["status"][3] == J.TRANSLATION
    scene["parts_count"] = 53
    scene["status"][5] = J.EMPTY
    scene["omega"], scene["velocity"] = 0.3 * scene["omega"], 0.05 * scene["velocity"]
    return Scene(dev, scene)


@pytest.mark.parametrize("per_problem", (False, True))
def test_blocks_with_every_kind_of_row(dev, blocks, per_problem):
    m, n, count = 3, blocks.xyz.shape[0], blocks.count
    assert n > count
    rng = np.random.default_rng(5)
    planted = (0.3 * rng.uniform(-1, 1, (m, 4))).astype(np.float32)
    targets = blocks.targets(planted)
    targets[:, count:] = np.nan                                     # padding past the count: never read as numbers
    weights = rng.uniform(0.2, 3.0, size=(m, n) if per_problem else (n,)).astype(np.float32)
    flat = weights.reshape(-1)
    flat[rng.choice(flat.size, 40, replace=False)] = 0.0
    flat[rng.choice(flat.size, 40, replace=False)] = -1.5
    flat[rng.choice(flat.size, 40, replace=False)] = np.nan
    flat[rng.choice(flat.size, 5, replace=False)] = np.inf
    targets[1, rng.choice(count, 25, replace=False)] = np.nan
    fit = blocks.solve(targets, weights=weights)
    ref, energy, total = _check_moments(blocks, fit, targets, weights)
    status = _np(fit.part_status)
    assert status[53] == 1 and status[5] == 1 and status[3] == 0 and _np(fit.depth).max() >= 3
    assert not ref[:, 5].any() and not ref[:, 53].any() and ref[:, 3, 0].all()
    slot = J.slots(blocks.labels, blocks.parts, 53, count)
    assert (blocks.labels[:count] == -1).any() and (blocks.labels[:count] == blocks.scene["outside_label"]).any() and (slot == 5).any()
    _check_honesty(blocks, fit, targets, weights=weights, energy=energy, total=total)
    _check_quality(blocks, fit, targets, energy, total, range(m), weights=weights)
    assert not fit.status.any() and (_np(fit.cost) <= COST_TOL * energy / total).all()


# ---- several chunks of rows, A = 10, no tree ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", (3240, 3239))
def test_a_face(dev, rows):
    scene = J.face()
    scene["omega"], scene["velocity"] = 0.3 * scene["omega"], 0.05 * scene["velocity"]
    scene["count"] = rows
    s = Scene(dev, scene, tree=False)
    assert s.xyz.shape[0] == 3240 and s.twists["omega"].shape[1] == 10
    planted = (0.2 * np.random.default_rng(6).uniform(-1, 1, (2, 10))).astype(np.float32)
    targets = s.targets(planted)
    fit = s.solve(targets)
    _, energy, total = _check_moments(s, fit, targets)
    assert fit.weight.tolist() == [float(rows)] * 2
    _check_honesty(s, fit, targets, energy=energy, total=total)
    _check_quality(s, fit, targets, energy, total, range(2))
    print("face: steps", fit.steps.tolist(), "cost / (E / W)", (_np(fit.cost) / (energy / total)).tolist())
    assert not fit.status.any() and (_np(fit.cost) <= COST_TOL * energy / total).all()


# ---- a line of 256 parts with 17 points each: two chunks of rows, K = 256, depth 255, and trees that are not trees ----------------------------
def _line(dev):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldJoints
    scene, joints, tree = R.line()
    tw = J.field_twists(dict(scene, weight=np.ones(256), energy=np.zeros((256, 3))), dev)
    t = lambda v, dtype: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).to(dev)   # noqa: E731
    j = joints["part_a"].shape[0]
    fj = FieldJoints(grid=FieldGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2)), labels=tw.labels, part_a=t(joints["part_a"], torch.int32),
                     part_b=t(joints["part_b"], torch.int32), contacts=torch.ones(j, dtype=torch.int64, device=dev),
                     status=torch.zeros(j, dtype=torch.int32, device=dev), count=_one(dev, joints["count"]),
                     anchor=t(joints["anchor"], torch.float64), omega=t(joints["omega"], torch.float64),
                     velocity=t(joints["velocity"], torch.float64), twists=tw)
    rng = np.random.default_rng(9)
    order = rng.permutation(256 * 17)                                                   # the parts' rows lie scattered over both chunks
    labels = np.repeat(np.arange(256, dtype=np.int32), 17)[order]
    xyz = (scene["centroid"][labels] + 0.02 * rng.normal(size=(labels.shape[0], 3))).astype(np.float32)
    return Scene(dev, scene, given=(tw, fj, tuple(t(v, torch.int32) for v in tree), xyz, labels))


def test_a_line_of_256_parts_and_trees_that_are_not_trees(dev):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import part_poses
    s = _line(dev)
    assert s.xyz.shape[0] == 4352 > hip.FIELD_TWISTS_CHUNK
    planted = (0.5 * np.random.default_rng(7).uniform(-1, 1, (1, 3))).astype(np.float32)
    targets = s.targets(planted)
    fit = s.solve(targets, iterations=3)
    _, energy, total = _check_moments(s, fit, targets)
    assert fit.depth.tolist() == list(range(256)) and not fit.part_status.any() and fit.weight.tolist() == [4352.0]
    _check_honesty(s, fit, targets, energy=energy, total=total)
    assert float(fit.cost) < float(fit.initial_cost) and int(fit.steps) >= 1
    # the line closed into a cycle: every slot has status 2, no row is counted, the kernel ends
    good = s.tree
    s.tree = (good[0].clone(), good[1].clone())
    s.tree[0][0] = 255
    s.refresh()
    cyc = s.solve(targets, init=np.float32([[0.1, 0.2, 0.3]]))
    _check_moments(s, cyc, targets)
    assert (cyc.part_status == 2).all() and cyc.status.tolist() == [F.NO_ROWS] and not cyc.moments.any()
    assert _np(cyc.commands).tolist() == [[np.float32(0.1), np.float32(0.2), np.float32(0.3)]]
    pose = part_poses(s.tw, cyc.commands, joints=s.joints, tree=s.tree)
    assert torch.equal(pose.status, cyc.part_status) and torch.equal(pose.depth, cyc.depth)
    # one bad link in the middle: the slots above it are excluded, the rest is solved
    s.tree = (good[0].clone(), good[1].clone())
    s.tree[1][200] = 7                                                                  # a joint that does not join 199 and 200
    s.refresh()
    cut = s.solve(targets, iterations=2)
    _, energy, total = _check_moments(s, cut, targets)
    assert cut.part_status.tolist() == [0] * 200 + [2] * 56 and cut.weight.tolist() == [200.0 * 17] and not cut.moments[0, 200:].any()
    _check_honesty(s, cut, targets, energy=energy, total=total)
    pose = part_poses(s.tw, cut.commands, joints=s.joints, tree=s.tree)
    assert torch.equal(pose.status, cut.part_status) and torch.equal(pose.depth, cut.depth)


# ---- the phases one by one -----------------------------------------------------------------------------------------------------------
def _raw(s, targets, out, phase, **kw):
    from neural_jacobian_field_amd import hip
    dev = s.dev
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)   # noqa: E731
    j = s.joints
    links = dict(part_a=j.part_a, part_b=j.part_b, count=j.count, anchor=j.anchor, omega=j.omega, velocity=j.velocity,
                 parent=s.tree[0], joint_of=s.tree[1])
    points = dict(xyz=t(s.xyz), labels=t(s.labels), count=_one(dev, s.count), targets=t(targets))
    hip.field_commands(s.tw.labels, s.tw.status, s.tw.centroid, s.tw.omega, s.tw.velocity, points, out, parts_count=s.tw.count,
                       joints=links, phase=phase, **kw)


def _buffers(dev, m, k, a_dim, sentinel):
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    return dict(commands=torch.full((m, a_dim), sentinel, dtype=torch.float32, device=dev), cost=torch.full((m,), sentinel, **f64),
                initial_cost=torch.full((m,), sentinel, **f64), weight=torch.full((m,), sentinel, **f64),
                steps=torch.full((m,), int(sentinel), **i32), gradient=torch.full((m, a_dim), sentinel, **f64),
                status=torch.full((m,), int(sentinel), **i32), part_status=torch.full((k,), int(sentinel), **i32),
                depth=torch.full((k,), int(sentinel), **i32), moments=torch.full((m, k, 23), sentinel, **f64))


def test_the_phases_one_by_one_and_every_output_is_written(dev, blocks):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldCommands
    m, count = 2, blocks.count
    planted = (0.3 * np.random.default_rng(11).uniform(-1, 1, (m, 4))).astype(np.float32)
    targets = blocks.targets(planted)
    sentinel = -12345.0
    out = _buffers(dev, m, 54, 4, sentinel)
    _raw(blocks, targets, out, hip.FIELD_COMMANDS_MOMENTS)
    assert all((out[f] == sentinel).all() for f in OUTPUTS if f not in ("moments", "part_status", "depth"))     # the solver has not run
    assert not any((out[f] == sentinel).any() for f in ("moments", "part_status", "depth"))
    device_moments = out["moments"].clone()
    exact, energy, total = _check_moments(blocks, FieldCommands(**out), targets)
    # the restatement's moments into the solver phase
    out["moments"].copy_(torch.from_numpy(exact))
    _raw(blocks, targets, out, hip.FIELD_COMMANDS_SOLVE)
    assert not any((out[f] == sentinel).any() for f in OUTPUTS)
    fed = FieldCommands(**out)
    _check_honesty(blocks, fed, targets, energy=energy, total=total)
    assert (_np(fed.cost) <= COST_TOL * energy / total).all()
    # the device's moments into the restatement
    back = blocks.restatement(targets, given_moments=_np(device_moments))
    assert (back["cost"] <= COST_TOL * energy / total).all() and np.abs(back["commands"] - _np(fed.commands)).max() <= 1e-6
    # both phases in one call: the bytes of the two calls, moments included
    both = _buffers(dev, m, 54, 4, sentinel)
    _raw(blocks, targets, both, hip.FIELD_COMMANDS_ALL)
    assert torch.equal(both["moments"].view(torch.uint8), device_moments.view(torch.uint8))
    assert not any((both[f] == sentinel).any() for f in OUTPUTS)
    assert np.abs(_np(both["commands"]) - _np(fed.commands)).max() <= 1e-6


# ---- determinism and capture -------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_a_capture_replays_them(dev, blocks):
    from neural_jacobian_field_amd.field_volume import FieldPointCloud, cloud_commands
    n, count = blocks.xyz.shape[0], blocks.count
    planted = (0.3 * np.random.default_rng(12).uniform(-1, 1, (20, 4))).astype(np.float32)
    targets = torch.from_numpy(blocks.targets(planted) + np.float32(0.01)).to(dev)
    cloud = FieldPointCloud(grid=_grid(blocks.scene), index=torch.from_numpy(blocks.scene["index"]).to(dev),
                            xyz=torch.from_numpy(blocks.xyz).to(dev), density=torch.ones(n, device=dev), color=None, jacobian=None,
                            count=_one(dev, count))
    labels = torch.from_numpy(blocks.labels).to(dev)
    kw = dict(joints=blocks.joints, tree=blocks.tree, lower=-0.25, upper=torch.full((4,), 0.25, device=dev), reg=1e-4)
    first, second = (cloud_commands(cloud, labels, blocks.tw, targets, **kw) for _ in range(2))
    for f in OUTPUTS:
        assert torch.equal(getattr(first, f).view(torch.uint8), getattr(second, f).view(torch.uint8)), f
    direct = blocks.solve(_np(targets), lower=-0.25, upper=0.25, reg=1e-4)
    assert torch.equal(direct.commands, first.commands) and torch.equal(direct.moments, first.moments)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fit = cloud_commands(cloud, labels, blocks.tw, targets, **kw)
    for f in OUTPUTS:
        getattr(fit, f).zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f in OUTPUTS:
        assert torch.equal(getattr(fit, f).view(torch.uint8), getattr(first, f).view(torch.uint8)), f
    assert int(first.steps.max()) >= 1


# ---- end to end: a model's field, its parts, their twists, joints and poses, and back to the commands -------------------------------------------
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


def test_cloud_commands_end_to_end(model, dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_commands, cloud_components, cloud_joints, cloud_pose,
                                                        cloud_twists, dominant_joint, extract_field)
    grid = FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), (17, 13, 11))
    c2w = synthetic.general_pose(7, 2, scale=0.04)
    c2w[0] = torch.eye(4)
    enc = PixelEncoding(features=synthetic.synthetic_features(2, IMG, IMG, seed=1).to(dev), extrinsics=c2w.to(dev),
                        intrinsics=synthetic.synthetic_cameras(2)["ctxt_k_norm"].to(dev), action=synthetic.synthetic_action(2, 8).to(dev))
    head, _ = model.compute_density(grid.points(device=dev)[None].expand(2, -1, 3).contiguous(), enc)
    cloud = extract_field(model, enc, grid, float(torch.quantile(head.density.reshape(-1).double().cpu(), 0.6)))
    labels, sizes, _ = cloud_components(cloud, keys=dominant_joint(cloud.jacobian))
    tw = cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=2, max_parts=64)
    joints = cloud_joints(cloud, labels, tw, batch=2)
    tree = joints.tree()
    speed = float(torch.linalg.vector_norm(tw.omega, dim=-1).max())
    u = torch.from_numpy((0.3 / max(speed, 1e-6) * np.random.default_rng(10).uniform(-1, 1, (5, 8))).astype(np.float32)).to(dev)
    _, posed = cloud_pose(cloud, labels, tw, u, joints=joints, tree=tree, first_order_elsewhere=False)
    count = int(cloud.count.item())
    posed[:, count:] = float("nan")                              # (cloud_pose leaves the rows past the count unwritten)
    fit = cloud_commands(cloud, labels, tw, posed, joints=joints, tree=tree)
    print(f"{count} rows, {int(tw.count.item())} parts: cost {fit.initial_cost.tolist()} -> {fit.cost.tolist()} in {fit.steps.tolist()} steps")
    assert (fit.cost <= fit.initial_cost).all() and not fit.status.any()
    for f in OUTPUTS:
        assert torch.isfinite(getattr(fit, f).double()).all(), f
