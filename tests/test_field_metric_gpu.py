"""GPU tests of inverse kinematics with a 3 x 3 information per target (field_volume.solve_commands_metric, ray_targets,
register_commands_metric; njf_field_commands_metric) against the numpy restatement of its semantics
(tests/field_metric_restatement.py), on the scheme and with the bounds of tests/test_field_commands_gpu.py.

(a) Moments: per entry ``|dev - ref| <= (n_p + 3) 2^-53 sum |terms|`` against the exactly rounded sums, in BOTH finishing forms (the
reduce-scatter and the butterflies, which must also agree byte for byte: a finished sum is the same tree over the lanes).
(b) Honesty: the device's cost, initial cost and gradient against the restatement's sums over the ROWS at the device's own
commands: ``|d cost| <= 1e-13 E / W``, ``|d g|_inf <= 1e-12 max(1, |g_0|_inf)``, ``E = sum w tr(Q) (|x~|^2 + |y~|^2)``.
(c) Quality: five more iterations of the restatement from the device's commands lower L by at most ``1e-9 L + 2e-13 E / W``;
planted commands are recovered within 1e-5 (with fp32 information and fp32 foot points the cost's floor is near ``1e-10 E /
W``, so no planted case is asked to end below ``2e-13 E / W``).
(d) The phases one by one, (e) trees that are not trees, (f) equal bytes and a captured replay, (g) the registration.

Observed on an MI355X: moments 0.23 of the bound at worst (the line), honesty 7e-4 (cost) and below 5e-5 (gradient), quality 0 or
1 further steps; single cameras 4 and 40 extents away end within 1e-5 of the planted commands at a cost of 4e-9 to 2e-8 E / W,
which is the pull of the helpers' floor (field_volume.INFORMATION_FLOOR).

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_commands_restatement as F
import field_joints_restatement as J
import field_metric_restatement as M
import field_pose_restatement as R
from neural_jacobian_field_amd.field_volume import FieldMetricCommands, solve_commands_metric  # noqa: F401  (what is under test)
from test_field_commands_gpu import Scene, _line

pytestmark = pytest.mark.gpu

COST_TOL = 2e-13
RECOVERY = 1e-5
OUTPUTS = ("commands", "cost", "initial_cost", "weight", "steps", "gradient", "status", "part_status", "depth", "moments")
NEAR = ("index", "distance2", "matched", "found")
HISTORY = ("commands_history", "cost_history", "found_history")
SIDES = ((1.0, 0.2, 0.3), (0.2, 1.0, -0.3), (0.3, -0.2, 1.0))              # the three sides of the host-side test


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _t(dev, v):
    return None if v is None else (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _count(s):
    return None if s.count is None else torch.tensor([s.count], dtype=torch.int32, device=s.dev)


def _solve(s, targets, information, weights=None, **kw):
    from neural_jacobian_field_amd.field_volume import solve_commands_metric
    kw = {k: _t(s.dev, v) for k, v in kw.items()}
    return solve_commands_metric(s.tw, _t(s.dev, s.xyz), _t(s.dev, s.labels), _t(s.dev, targets), _t(s.dev, information), joints=s.joints,
                                 tree=s.tree, weights=_t(s.dev, weights), count=_count(s), **kw)


def _restatement(s, targets, information, **kw):
    return M.solve(s.twists, s.xyz, s.labels, targets, information, s.parts, s.jd, s.td, count=s.count, **kw)


def _buffers(dev, m, k, a_dim, sentinel):
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    return dict(commands=torch.full((m, a_dim), sentinel, dtype=torch.float32, device=dev), cost=torch.full((m,), sentinel, **f64),
                initial_cost=torch.full((m,), sentinel, **f64), weight=torch.full((m,), sentinel, **f64),
                steps=torch.full((m,), int(sentinel), **i32), gradient=torch.full((m, a_dim), sentinel, **f64),
                status=torch.full((m,), int(sentinel), **i32), part_status=torch.full((k,), int(sentinel), **i32),
                depth=torch.full((k,), int(sentinel), **i32), moments=torch.full((m, k, M.MOMENTS), sentinel, **f64))


def _raw(s, targets, information, out, phase, weights=None, **kw):
    from neural_jacobian_field_amd import hip
    j = s.joints
    links = None if j is None else dict(part_a=j.part_a, part_b=j.part_b, count=j.count, anchor=j.anchor, omega=j.omega,
                                        velocity=j.velocity, parent=s.tree[0], joint_of=s.tree[1])
    points = dict(xyz=_t(s.dev, s.xyz), labels=_t(s.dev, s.labels), count=_count(s), targets=_t(s.dev, targets),
                  information=_t(s.dev, information))
    hip.field_commands_metric(s.tw.labels, s.tw.status, s.tw.centroid, s.tw.omega, s.tw.velocity, points, out, parts_count=s.tw.count,
                              joints=links, weights=_t(s.dev, weights), phase=phase, **kw)


def _pick(v, problems, m):
    """The rows ``problems`` of a per-problem array, or a shared one as it is."""
    return v if v is None or v.shape[0] != m or v.ndim < 2 else v[problems]


def _check_moments(s, fit, targets, information, weights=None, problems=None):
    """(a): the device's moments of ``problems`` against the exactly rounded sums; returns ``(moments, E, W)`` of those problems."""
    m = targets.shape[0]
    problems = list(range(m)) if problems is None else list(problems)
    status, depth = F.pose_status(s.twists, s.jd, s.td)
    assert np.array_equal(_np(fit.part_status), status) and np.array_equal(_np(fit.depth), depth)
    q = M.per_problem(information, m)[problems]
    w = weights if weights is None or weights.ndim == 1 else weights[problems]
    ref, bound = M.moments(s.xyz, s.labels, targets[problems], q, s.parts, s.twists["count"], status, s.twists["centroid"], w, s.count)
    got = _np(fit.moments)
    assert got.shape == (m, len(s.parts), M.MOMENTS) and fit.moments.dtype == torch.float64
    err = np.abs(got[problems] - ref)
    ratio = (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0
    print(f"moments: worst ratio to the bound {ratio:.4f} over {int((bound > 0).sum())} entries; {int((ref[..., 0] > 0).sum())} (m, p) with rows")
    assert (err <= bound).all()                                  # (an entry without a term has bound 0: it must be exactly 0)
    energy, total = M.energy(s.xyz, s.labels, targets[problems], q, s.parts, s.twists["count"], status, s.twists["centroid"], w, s.count)
    return ref, energy, total


def _check_honesty(s, fit, targets, information, energy, total, problems, weights=None, init=None, lower=None, upper=None, reg=0.0):
    """(b): cost, initial cost and gradient against the restatement's sums over the rows at the device's own commands."""
    m, a_dim = targets.shape[0], s.twists["omega"].shape[1]
    q = M.per_problem(information, m)
    slot, w = M.counted(s.xyz, s.labels, targets, q, s.parts, s.twists["count"], _np(fit.part_status), weights, s.count)
    commands = _np(fit.commands)
    assert commands.dtype == np.float32 and commands.shape == (m, a_dim)
    box = lambda v, fill: np.broadcast_to(np.float32(fill if v is None else v), (m, a_dim))   # noqa: E731
    start = np.minimum(np.maximum(box(init, 0.0), box(lower, -np.inf)), box(upper, np.inf)).astype(np.float32)
    worst = [0.0, 0.0]
    for at, i in enumerate(problems):
        if _np(fit.status)[i]:
            continue
        first = M.evaluate_rows(s.xyz, slot, w[i], targets[i], q[i], F.chain(s.twists, start[i], s.jd, s.td))
        last = M.evaluate_rows(s.xyz, slot, w[i], targets[i], q[i], F.chain(s.twists, commands[i], s.jd, s.td))
        scale = energy[at] / total[at]
        g0 = np.abs(first[1] + reg / a_dim * start[i].astype(np.float64)).max()
        g = last[1] + reg / a_dim * commands[i].astype(np.float64)
        dc = max(abs(_np(fit.cost)[i] - max(last[0], 0.0)), abs(_np(fit.initial_cost)[i] - max(first[0], 0.0))) / (1e-13 * scale)
        dg = np.abs(_np(fit.gradient)[i] - g).max() / (1e-12 * max(1.0, g0))
        worst = [max(worst[0], dc), max(worst[1], dg)]
        assert abs(_np(fit.weight)[i] - last[3]) <= 1e-12 * last[3]
    print(f"honesty: worst ratio to the bound, cost {worst[0]:.4f}, gradient {worst[1]:.4f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def _check_quality(s, fit, targets, information, energy, total, problems, **kw):
    """(c): five more iterations of the restatement from the device's commands lower L by at most 1e-9 L + 2e-13 E / W."""
    m = targets.shape[0]
    problems = list(problems)
    sub = {k: _pick(v, problems, m) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    more = _restatement(s, targets[problems], M.per_problem(information, m)[problems], init=_np(fit.commands)[problems], iterations=5, **sub)
    a_dim = s.twists["omega"].shape[1]
    reg = kw.get("reg", 0.0)
    for at, i in enumerate(problems):
        u0, u1 = _np(fit.commands)[i].astype(np.float64), more["commands"][at].astype(np.float64)
        before = more["initial_cost"][at] + reg / a_dim * (u0 @ u0)
        after = more["cost"][at] + reg / a_dim * (u1 @ u1)
        print(f"quality: problem {i}: L {before:.3e} -> {after:.3e} in {more['steps'][at]} more steps; E / W {energy[at] / total[at]:.3e}")
        assert before - after <= 1e-9 * before + COST_TOL * energy[at] / total[at]


def _slid(moved, rng, amount):
    """(targets, information [.., 6], normals): every moved row slid by ``amount`` inside a plane of a random unit normal."""
    normals = rng.normal(size=moved.shape)
    normals = (normals / np.linalg.norm(normals, axis=-1, keepdims=True)).astype(np.float32)
    n64 = normals.astype(np.float64)
    slide = np.cross(n64, rng.normal(size=moved.shape))
    slide -= n64 * (slide * n64).sum(axis=-1, keepdims=True) / (n64 * n64).sum(axis=-1, keepdims=True)
    slide *= amount / np.linalg.norm(slide, axis=-1, keepdims=True)
    return (moved.astype(np.float64) + slide).astype(np.float32), M.plane_information(normals), normals


def _spoil(rng, n, count, targets, information, labels):
    """Every kind of row that is left out, mixed into copies of the inputs: ``(targets, information [M, n, 6], weights [M, n],
    labels)``."""
    m = targets.shape[0]
    targets, information, labels = targets.copy(), M.per_problem(information, m).copy(), labels.copy()
    weights = rng.uniform(0.2, 3.0, size=(m, n)).astype(np.float32)
    flat = weights.reshape(-1)
    for value in (0.0, -1.5, np.nan, np.inf):
        flat[rng.choice(flat.size, max(4, flat.size // 60), replace=False)] = value
    for i in range(m):
        rows = rng.choice(count, max(3, count // 40), replace=False)
        information[i, rows, rng.integers(0, 6, rows.size)] = np.nan
        information[i, rng.choice(count, 2, replace=False), 3] = np.inf
        targets[i, rng.choice(count, max(3, count // 40), replace=False), rng.integers(0, 3)] = np.nan
    labels[rng.choice(count, max(3, count // 50), replace=False)] = 9999          # the label of no part
    targets[:, count:] = np.nan                                                # rows beyond the count: never read as numbers
    information[:, count:] = np.nan
    return targets, information, weights, labels


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(dev):
    return Scene(dev, J.chain())


@pytest.fixture(scope="module")
def line(dev):
    return _line(dev)


@pytest.fixture(scope="module")
def face(dev):
    scene = J.face()
    scene["omega"], scene["velocity"] = 0.3 * scene["omega"], 0.05 * scene["velocity"]
    return Scene(dev, scene, tree=False)


CASES = {"chain": (5, 260, (0, 3, 4)), "line": (17, 4300, (0, 15, 16)), "face": (2, 3239, (0, 1))}


# ---- (a) the moments, in both finishing forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_problem", (False, True))
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_moments_in_both_finishing_forms(dev, request, case, per_problem):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldMetricCommands
    s = request.getfixturevalue(case)
    m, count, problems = CASES[case]
    n, k, a_dim = s.xyz.shape[0], len(s.parts), s.twists["omega"].shape[1]
    assert n > count and (case != "line" or n > hip.FIELD_TWISTS_CHUNK) and (case != "chain" or (n, k) == (272, 3))
    rng = np.random.default_rng(50 + per_problem)
    planted = (0.3 * rng.uniform(-1, 1, (m, a_dim))).astype(np.float32)
    moved = s.targets(planted)
    a = rng.normal(size=((m, n) if per_problem else (n,)) + (3, 3))
    information = M.pack(a @ np.swapaxes(a, -1, -2))                         # random symmetric positive semi-definite matrices
    keep = (s.count, s.labels)
    try:
        s.count = count
        targets, spoiled, weights, s.labels = _spoil(rng, n, count, moved, information, s.labels)
        if not per_problem:                                                  # one table for every problem: spoil it once
            spoiled = spoiled[0]
        out = {}
        for name, modifier in (("scatter", 0), ("butterfly", hip.FIELD_COMMANDS_METRIC_BUTTERFLY)):
            out[name] = _buffers(dev, m, k, a_dim, -12345.0)
            _raw(s, targets, spoiled, out[name], hip.FIELD_COMMANDS_MOMENTS | modifier, weights=weights)
            assert all((out[name][f] == -12345.0).all() for f in OUTPUTS if f not in ("moments", "part_status", "depth"))
            assert not any((out[name][f] == -12345.0).any() for f in ("moments", "part_status", "depth"))
            print(case, name, end=": ")
            ref, _, _ = _check_moments(s, FieldMetricCommands(**out[name]), targets, spoiled, weights, problems)
        assert torch.equal(_bytes(out["scatter"]["moments"]), _bytes(out["butterfly"]["moments"]))       # the same tree over the lanes
        status, _ = F.pose_status(s.twists, s.jd, s.td)
        _, every = F.counted(s.xyz, s.labels, moved, s.parts, s.twists["count"], status, None, None)
        _, kept = M.counted(s.xyz, s.labels, targets, spoiled, s.parts, s.twists["count"], status, weights, count)
        left = (every > 0).sum(axis=1) - (kept > 0).sum(axis=1)
        print(case, "rows left out per problem:", left.tolist())
        assert (left >= 10).all() and (kept > 0).any(axis=1).all()
    finally:
        s.count, s.labels = keep


# ---- (b), (c) the solver ---------------------------------------------------------------------------------------------------------------
def _cameras(s, extents):
    from test_field_metric_cpu import _camera
    d = dict(xyz=s.xyz, labels=s.labels)
    pairs = [_camera(d, SIDES[i % 3], extents) for i in range(5)]        # five problems: the three sides, two of them twice
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


@pytest.mark.parametrize("extents", (4.0, 40.0))
def test_five_cameras_each_recover_the_planted_chain_from_pixels(dev, chain, extents):
    from neural_jacobian_field_amd import geometry
    from neural_jacobian_field_amd.field_volume import part_poses, ray_targets
    m = 5
    planted = np.float32([[0.6, -0.4, 0.0], [-0.5, 0.3, 0.0], [0.2, 0.6, 0.0], [0.9, -0.2, 0.0], [-0.3, -0.5, 0.0]])
    k, c2w = _cameras(chain, extents)
    pixels = M.project(chain.targets(planted), k, c2w).astype(np.float32)
    assert pixels.min() > 0.0 and pixels.max() < 1.0
    pixels[1, 7, 0] = np.nan                                               # a keypoint that was not seen: its row is free
    targets, information = ray_targets(*(_t(dev, v) for v in (chain.xyz, pixels, k, c2w)))
    want_t, want_q = M.ray_targets(chain.xyz, pixels, k, c2w)
    _, rays = geometry.get_world_rays(*(_t(dev, v) for v in (np.nan_to_num(pixels, nan=0.5), k, c2w)))
    excess = (_np(rays).astype(np.float64) ** 2).sum(axis=-1) - 1.0
    print(f"|d|^2 - 1 of the ray launch: {excess.min():.2e} .. {excess.max():.2e}; of the information: "
          f"{np.nanmin(2.0 - _np(information).astype(np.float64)[..., [0, 3, 5]].sum(axis=-1)):.2e} .. "
          f"{np.nanmax(2.0 - _np(information).astype(np.float64)[..., [0, 3, 5]].sum(axis=-1)):.2e}")
    assert targets.dtype == information.dtype == torch.float32 and targets.shape == (m, 272, 3) and information.shape == (m, 272, 6)
    free = np.isnan(want_t).all(axis=-1)
    assert free.sum() == 1 and np.array_equal(np.isnan(_np(targets)).all(axis=-1), free)
    scale = np.abs(c2w[:, :3, 3]).max()
    assert np.abs(_np(targets)[~free] - want_t[~free]).max() <= 16 * 2.0 ** -23 * scale
    assert np.abs(_np(information)[~free] - want_q[~free]).max() <= 8 * 2.0 ** -23
    # every matrix is positive semi-definite in fp32: the floor of ray_information holds on the device's own directions
    assert np.linalg.eigvalsh(M.symmetric(_np(information)[~free])).min() > 0.0
    start = np.zeros((m, 3), np.float32)
    start[:, 2] = np.linspace(-1.0, 1.0, m, dtype=np.float32)
    fit = _solve(chain, targets, information, init=start)
    for f, shape, dtype in (("commands", (m, 3), torch.float32), ("cost", (m,), torch.float64), ("initial_cost", (m,), torch.float64),
                            ("weight", (m,), torch.float64), ("steps", (m,), torch.int32), ("gradient", (m, 3), torch.float64),
                            ("status", (m,), torch.int32), ("part_status", (3,), torch.int32), ("depth", (3,), torch.int32),
                            ("moments", (m, 3, 74), torch.float64)):
        t = getattr(fit, f)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cuda", f
    targets, information = _np(targets), _np(information)
    _, energy, total = _check_moments(chain, fit, targets, information)
    assert fit.weight.tolist() == [272.0, 271.0, 272.0, 272.0, 272.0] and not fit.status.any() and fit.depth.tolist() == [0, 1, 2]
    _check_honesty(chain, fit, targets, information, energy, total, range(m), init=start)
    print(f"pixels at {extents} extents: steps {fit.steps.tolist()}, |u - planted| {np.abs(_np(fit.commands)[:, :2] - planted[:, :2]).max():.2e}, "
          f"cost / (E / W) {(_np(fit.cost) / (energy / total)).tolist()}")
    assert _np(fit.commands)[:, 2].tobytes() == start[:, 2].tobytes()          # channel 2 moves nothing: bitwise its start
    assert np.abs(_np(fit.commands)[:, :2] - planted[:, :2]).max() <= RECOVERY
    assert torch.equal(fit.rms(), fit.cost.sqrt())
    _check_quality(chain, fit, targets, information, energy[[0, 1, 4]], total[[0, 1, 4]], (0, 1, 4))
    pose = part_poses(chain.tw, fit.commands, joints=chain.joints, tree=chain.tree)
    assert torch.equal(pose.status, fit.part_status) and torch.equal(pose.depth, fit.depth)


def test_planes_bounds_noise_and_the_regulariser_on_the_chain(dev, chain):
    m = 5
    rng = np.random.default_rng(61)
    planted = np.float32([[0.9, -0.7, 0.0], [0.5, 0.3, 0.0], [-0.8, 0.6, 0.0], [0.6, -0.4, 0.0], [0.1, 0.2, 0.0]])
    extent = float(np.linalg.norm(chain.xyz.max(axis=0) - chain.xyz.min(axis=0)))
    targets, information, _ = _slid(chain.targets(planted), rng, 0.5 * extent)
    fit = _solve(chain, targets, information)
    from neural_jacobian_field_amd.field_volume import solve_commands
    point = solve_commands(chain.tw, _t(dev, chain.xyz), _t(dev, chain.labels), _t(dev, targets), joints=chain.joints, tree=chain.tree)
    print("planes:", np.abs(_np(fit.commands) - planted).max(), "points:", np.abs(_np(point.commands) - planted).max())
    assert np.abs(_np(fit.commands) - planted).max() <= RECOVERY and np.abs(_np(point.commands) - planted).max(axis=1).min() > 1e-2
    _, energy, total = _check_moments(chain, fit, targets, information)
    _check_honesty(chain, fit, targets, information, energy, total, range(m))
    boxed = _solve(chain, targets, information, lower=-0.5, upper=torch.tensor([0.5, 0.5, 0.5], device=dev))
    assert _np(boxed.commands)[0].tolist() == [0.5, -0.5, 0.0]
    g = _np(boxed.gradient)[0]
    assert g[0] < 0.0 and g[1] > 0.0 and g[2] == 0.0
    _check_honesty(chain, boxed, targets, information, energy, total, range(m), lower=-0.5, upper=0.5)
    _check_quality(chain, boxed, targets, information, energy[:3], total[:3], range(3), lower=-0.5, upper=0.5)
    noisy = (targets + 0.02 * rng.normal(size=targets.shape)).astype(np.float32)
    for reg in (0.0, 1e-3):
        fit = _solve(chain, noisy, information, reg=reg)
        _, energy, total = _check_moments(chain, fit, noisy, information)
        _check_honesty(chain, fit, noisy, information, energy, total, range(m), reg=reg)
        _check_quality(chain, fit, noisy, information, energy[[0, 2, 4]], total[[0, 2, 4]], (0, 2, 4), reg=reg)
        assert (_np(fit.cost) <= _np(fit.initial_cost)).all()
    free, held = _solve(chain, targets, information), _solve(chain, targets, information, reg=1e-3)
    assert (torch.linalg.vector_norm(held.commands, dim=1) < torch.linalg.vector_norm(free.commands, dim=1)).all()
    # the identity information is solve_commands' objective
    identity = np.broadcast_to(M.IDENTITY6, (272, 6)).copy()
    same = _solve(chain, noisy, identity)
    theirs = solve_commands(chain.tw, _t(dev, chain.xyz), _t(dev, chain.labels), _t(dev, noisy), joints=chain.joints, tree=chain.tree)
    assert np.abs(_np(same.commands) - _np(theirs.commands)).max() <= 1e-6
    _, energy, total = _check_moments(chain, same, noisy, identity)
    assert (np.abs(_np(same.cost) - _np(theirs.cost)) <= 1e-13 * energy / total).all() and torch.equal(same.weight, theirs.weight)


def test_handles_and_empty_problems(dev, chain):
    planted = np.float32([[0.6, -0.4, 0.0]] * 5)
    full = chain.targets(planted)
    tip = np.flatnonzero(chain.labels == chain.parts[2])
    targets = np.full_like(full, np.nan)
    information = np.broadcast_to(M.IDENTITY6, (5, 272, 6)).copy()
    targets[0, tip[[0, 5, 40, 63]]] = full[0, tip[[0, 5, 40, 63]]]
    targets[1, tip[17]] = full[1, tip[17]]
    targets[3, tip[3]] = full[3, tip[3]]
    information[3, tip[3], 4] = np.nan                                  # one NaN information entry: the row is not counted
    targets[4] = full[4]
    information[4] = 0.0                                                # no information at all: every row counts and nothing pulls
    start = np.float32([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.2, -3.0, 1.0], [0.1, 0.1, 0.1], [0.3, 0.2, 0.1]])
    fit = _solve(chain, targets, information, init=start, lower=-1.0, upper=1.0)
    assert fit.status.tolist() == [0, 0, F.NO_ROWS, F.NO_ROWS, 0] and fit.weight.tolist() == [4.0, 1.0, 0.0, 0.0, 272.0]
    assert _np(fit.commands)[2].tolist() == [np.float32(0.2), -1.0, 1.0] and _np(fit.commands)[3:].tobytes() == start[3:].tobytes()
    assert not fit.cost[2:].any() and not fit.steps[2:].any() and not fit.moments[2:4].any() and not fit.gradient[2:].any()
    _, energy, total = _check_moments(chain, fit, targets, information)
    _check_honesty(chain, fit, targets, information, energy, total, (0, 1), init=start, lower=-1.0, upper=1.0)
    assert np.abs(_np(fit.commands)[:2] - planted[:2]).max() <= RECOVERY
    not_finite = _solve(chain, full[:1], information[0], init=np.float32([[np.inf, 0.0, 0.0]]))
    assert not_finite.status.tolist() == [F.NOT_FINITE] and not_finite.steps.tolist() == [0]
    assert _np(not_finite.commands)[0].tolist() == [np.inf, 0.0, 0.0]


@pytest.mark.parametrize("rows", (3240, 3239))
def test_a_face(dev, face, rows):
    keep = face.count
    try:
        face.count = rows
        rng = np.random.default_rng(6)
        planted = (0.2 * rng.uniform(-1, 1, (2, 10))).astype(np.float32)
        targets, information, _ = _slid(face.targets(planted), rng, 0.05)
        fit = _solve(face, targets, information)
        _, energy, total = _check_moments(face, fit, targets, information)
        assert fit.weight.tolist() == [float(rows)] * 2 and not fit.status.any()
        _check_honesty(face, fit, targets, information, energy, total, range(2))
        _check_quality(face, fit, targets, information, energy, total, range(2))
        print("face: steps", fit.steps.tolist(), "cost / (E / W)", (_np(fit.cost) / (energy / total)).tolist(),
              "|u - planted|", np.abs(_np(fit.commands) - planted).max())
        assert (_np(fit.cost) < _np(fit.initial_cost)).all()
    finally:
        face.count = keep


# ---- (e) a line of 256 parts, and trees that are not trees --------------------------------------------------------------------------------
def test_a_line_of_256_parts_and_trees_that_are_not_trees(dev, line):
    from neural_jacobian_field_amd.field_volume import part_poses
    s, m, problems = line, 17, (0, 15, 16)
    rng = np.random.default_rng(7)
    planted = (0.5 * rng.uniform(-1, 1, (m, 3))).astype(np.float32)
    targets, information, _ = _slid(s.targets(planted), rng, 0.05)
    fit = _solve(s, targets, information, iterations=3)
    _, energy, total = _check_moments(s, fit, targets, information, problems=problems)
    assert fit.depth.tolist() == list(range(256)) and not fit.part_status.any() and fit.weight.tolist() == [4352.0] * m
    _check_honesty(s, fit, targets, information, energy, total, problems)
    assert (fit.cost < fit.initial_cost).all() and int(fit.steps.min()) >= 1
    good = s.tree
    try:
        # the line closed into a cycle: every slot has status 2, no row is counted, the kernel ends
        s.tree = (good[0].clone(), good[1].clone())
        s.tree[0][0] = 255
        s.refresh()
        start = np.float32([[0.1, 0.2, 0.3]] * m)
        cyc = _solve(s, targets, information, init=start)
        _check_moments(s, cyc, targets, information, problems=(0, 16))
        assert (cyc.part_status == 2).all() and cyc.status.tolist() == [F.NO_ROWS] * m and not cyc.moments.any()
        assert _np(cyc.commands).tobytes() == start.tobytes()
        pose = part_poses(s.tw, cyc.commands, joints=s.joints, tree=s.tree)
        assert torch.equal(pose.status, cyc.part_status) and torch.equal(pose.depth, cyc.depth)
        # one bad link in the middle: the slots above it are excluded, the rest is solved
        s.tree = (good[0].clone(), good[1].clone())
        s.tree[1][200] = 7                                                                  # a joint that does not join 199 and 200
        s.refresh()
        cut = _solve(s, targets, information, iterations=2)
        _, energy, total = _check_moments(s, cut, targets, information, problems=(16,))
        assert cut.part_status.tolist() == [0] * 200 + [2] * 56 and cut.weight.tolist() == [200.0 * 17] * m and not cut.moments[:, 200:].any()
        _check_honesty(s, cut, targets, information, energy, total, (16,))
        pose = part_poses(s.tw, cut.commands, joints=s.joints, tree=s.tree)
        assert torch.equal(pose.status, cut.part_status) and torch.equal(pose.depth, cut.depth)
    finally:
        s.tree = good
        s.refresh()


# ---- (d) the phases one by one ------------------------------------------------------------------------------------------------------------
def test_the_phases_one_by_one_and_every_output_is_written(dev, chain):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldMetricCommands
    m = 5
    rng = np.random.default_rng(11)
    planted = (0.5 * rng.uniform(-1, 1, (m, 3))).astype(np.float32)
    planted[:, 2] = 0.0
    targets, information, _ = _slid(chain.targets(planted), rng, 0.3)
    sentinel = -12345.0
    out = _buffers(dev, m, 3, 3, sentinel)
    _raw(chain, targets, information, out, hip.FIELD_COMMANDS_MOMENTS)
    assert all((out[f] == sentinel).all() for f in OUTPUTS if f not in ("moments", "part_status", "depth"))     # the solver has not run
    assert not any((out[f] == sentinel).any() for f in ("moments", "part_status", "depth"))
    device_moments = out["moments"].clone()
    exact, energy, total = _check_moments(chain, FieldMetricCommands(**out), targets, information)
    # the restatement's moments into the solver phase
    out["moments"].copy_(torch.from_numpy(exact))
    _raw(chain, targets, information, out, hip.FIELD_COMMANDS_SOLVE)
    assert not any((out[f] == sentinel).any() for f in OUTPUTS)
    fed = FieldMetricCommands(**out)
    _check_honesty(chain, fed, targets, information, energy, total, range(m))
    assert np.abs(_np(fed.commands) - planted).max() <= RECOVERY
    # the solver phase needs neither rows nor information
    alone = _buffers(dev, m, 3, 3, sentinel)
    alone["moments"].copy_(torch.from_numpy(exact))
    _raw(chain, np.full_like(targets, np.nan), np.full_like(information, np.nan), alone, hip.FIELD_COMMANDS_SOLVE)
    for f in OUTPUTS:
        assert torch.equal(_bytes(alone[f]), _bytes(out[f])), f
    # the device's moments into the restatement
    back = _restatement(chain, targets, information, given_moments=_np(device_moments))
    assert np.abs(back["commands"] - _np(fed.commands)).max() <= 1e-6 and np.abs(back["commands"] - planted).max() <= RECOVERY
    # both phases in one call, in either finishing form: the bytes of the two calls, moments included
    for modifier in (0, hip.FIELD_COMMANDS_METRIC_BUTTERFLY):
        both = _buffers(dev, m, 3, 3, sentinel)
        _raw(chain, targets, information, both, hip.FIELD_COMMANDS_ALL | modifier)
        assert torch.equal(_bytes(both["moments"]), _bytes(device_moments))
        assert not any((both[f] == sentinel).any() for f in OUTPUTS)
        assert np.abs(_np(both["commands"]) - _np(fed.commands)).max() <= 1e-6
    direct = _solve(chain, targets, information)
    for f in OUTPUTS:
        assert torch.equal(_bytes(getattr(direct, f)), _bytes(both[f])), f


# ---- (f) determinism and capture ---------------------------------------------------------------------------------------------------------
def _cloud(s):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud
    n = s.xyz.shape[0]
    grid = FieldGrid(s.scene["origin"], s.scene["step"], s.scene["dims"])
    return FieldPointCloud(grid=grid, index=_t(s.dev, s.scene["index"]), xyz=_t(s.dev, s.xyz), density=torch.ones(n, device=s.dev),
                           color=None, jacobian=None, count=torch.tensor([n if s.count is None else s.count], dtype=torch.int32, device=s.dev))


def test_two_calls_give_equal_bytes_and_a_capture_replays_them(dev, line, chain):
    from neural_jacobian_field_amd.field_volume import cloud_commands_metric, solve_commands_metric
    # the line: two chunks of rows and a second tile of problems
    rng = np.random.default_rng(12)
    planted = (0.5 * rng.uniform(-1, 1, (17, 3))).astype(np.float32)
    targets, information, _ = _slid(line.targets(planted), rng, 0.05)
    args = [_t(dev, v) for v in (line.xyz, line.labels, targets, information)]
    kw = dict(joints=line.joints, tree=line.tree, iterations=3, lower=-0.45, upper=torch.full((3,), 0.45, device=dev), reg=1e-4)
    first, second = (solve_commands_metric(line.tw, *args, **kw) for _ in range(2))
    for f in OUTPUTS:
        assert torch.equal(_bytes(getattr(first, f)), _bytes(getattr(second, f))), f
    assert int(first.steps.max()) >= 1
    # the chain as a cloud: captured and replayed
    cloud, labels = _cloud(chain), _t(dev, chain.labels)
    planted = (0.5 * rng.uniform(-1, 1, (5, 3))).astype(np.float32)
    targets, information, _ = _slid(chain.targets(planted), rng, 0.3)
    targets, information = _t(dev, targets), _t(dev, information[0])           # one table of information for the five problems
    kw = dict(joints=chain.joints, tree=chain.tree, lower=-0.45, upper=torch.full((3,), 0.45, device=dev), reg=1e-4)
    first = cloud_commands_metric(cloud, labels, chain.tw, targets, information, **kw)
    direct = _solve(chain, targets, information, lower=-0.45, upper=0.45, reg=1e-4)
    for f in OUTPUTS:
        assert torch.equal(_bytes(getattr(first, f)), _bytes(getattr(direct, f))), f
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fit = cloud_commands_metric(cloud, labels, chain.tw, targets, information, **kw)
    for f in OUTPUTS:
        getattr(fit, f).zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f in OUTPUTS:
        assert torch.equal(_bytes(getattr(fit, f)), _bytes(getattr(first, f))), f
    assert int(first.steps.max()) >= 1


# ---- (g) the registration ------------------------------------------------------------------------------------------------------------------
def _scene_cells(scene):
    from neural_jacobian_field_amd.field_volume import cell_grid
    upper = [o + s * (d - 1) for o, s, d in zip(scene["origin"], scene["step"], scene["dims"])]
    return cell_grid(scene["origin"], upper, max(scene["step"]))


def _loop(s, observed, observed_information, cells, reach, rounds, iterations, init=None, lower=None, upper=None, **kw):
    """The registration written from its public pieces."""
    from neural_jacobian_field_amd.field_volume import nearest_points, part_poses, solve_commands_metric
    dev = s.dev
    xyz, labels, count = _t(dev, s.xyz), _t(dev, s.labels), _count(s)
    mo = observed.shape[0] if observed.dim() == 3 else 1
    m = max(mo, 1 if init is None else init.shape[0])
    n, t = xyz.shape[0], observed.shape[-2]
    u = torch.zeros(m, s.twists["omega"].shape[1], device=dev) if init is None else init
    if lower is not None:
        u = torch.clamp(u, min=lower)
    if upper is not None:
        u = torch.clamp(u, max=upper)
    table = observed_information.reshape(-1, t, 6)
    history = []
    for _ in range(rounds):
        posed = part_poses(s.tw, u, joints=s.joints, tree=s.tree).apply(xyz, labels, count=count)
        near = nearest_points(posed, observed, cells, reach, count=count, labels=labels)
        rows = near.index.clamp(min=0).long()
        information = torch.stack([table[0 if table.shape[0] == 1 else i][rows[i]] for i in range(m)])
        assert information.shape == (m, n, 6)
        fit = solve_commands_metric(s.tw, xyz, labels, near.matched, information, joints=s.joints, tree=s.tree, count=count, init=u,
                                    lower=lower, upper=upper, iterations=iterations, **kw)
        history.append((fit.commands.clone(), fit.cost.clone(), near.found.clone()))
        u = fit.commands
    return fit, near, [torch.stack([h[i] for h in history]) for i in range(3)]


def _register(s, observed, observed_information, cells, reach, **kw):
    from neural_jacobian_field_amd.field_volume import register_commands_metric
    return register_commands_metric(s.tw, _t(s.dev, s.xyz), _t(s.dev, s.labels), observed, observed_information, cells, reach,
                                    joints=s.joints, tree=s.tree, count=_count(s), **kw)


def _same_registration(reg, fit, near, history):
    from neural_jacobian_field_amd.field_volume import FieldMetricCommands, FieldRegistration
    assert isinstance(reg, FieldRegistration) and isinstance(reg.fit, FieldMetricCommands)
    for f in OUTPUTS:
        assert torch.equal(_bytes(getattr(reg.fit, f)), _bytes(getattr(fit, f))), f
    for f in NEAR:
        assert torch.equal(_bytes(getattr(reg.matches, f)), _bytes(getattr(near, f))), f
    for f, h in zip(HISTORY, history):
        got = getattr(reg, f)
        assert got.dtype == h.dtype and got.shape == h.shape and torch.equal(_bytes(got), _bytes(h)), f


def _observation(s, commands, rng, surface=False):
    """(observed [M, n, 3], normals [M, n, 3]): the rows posed at ``commands`` in a shuffled order, with synthetic unit normals
    -- random ones, or with ``surface`` those of a smooth body around every posed part: the direction from the part's posed
    centroid to the point, as a cloud's estimated normals point away from the body."""
    posed = s.targets(commands)
    if surface:
        ref = R.poses(s.twists, np.asarray(commands, np.float32), s.jd, s.td)
        normals = np.zeros(posed.shape)
        for k, label in enumerate(s.parts):
            rows = s.labels == label
            centre = np.einsum("mij,j->mi", ref["rotation"][:, k], np.asarray(s.twists["centroid"][k])) + ref["translation"][:, k]
            normals[:, rows] = posed[:, rows] - centre[:, None, :]
        normals += 1e-3                                                        # (no point lies on its centroid after this)
    else:
        normals = rng.normal(size=posed.shape)
    normals = (normals / np.linalg.norm(normals, axis=-1, keepdims=True)).astype(np.float32)
    order = [rng.permutation(posed.shape[1]) for _ in posed]
    return np.stack([p[o] for p, o in zip(posed, order)]), np.stack([v[o] for v, o in zip(normals, order)])


@pytest.mark.parametrize("shared", (False, True))
def test_register_commands_metric_is_the_loop_of_its_public_pieces(dev, chain, shared):
    from neural_jacobian_field_amd.field_volume import plane_information
    rng = np.random.default_rng(40 + shared)
    m = 3
    planted = np.float32([[0.25, -0.2, 0.0], [-0.4, 0.1, 0.0], [0.1, 0.2, 0.0]])
    observed, normals = _observation(chain, planted[:1] if shared else planted, rng)
    if shared:                                                                 # one observation [T, 3] and one table [T, 6], three starts
        observed, normals = observed[0], normals[0]
    observed, information = _t(dev, observed), plane_information(_t(dev, normals))
    assert information.shape == observed.shape[:-1] + (6,)
    cells, reach = _scene_cells(chain.scene), 4 * chain.scene["step"][0]
    kw = dict(rounds=4, iterations=2, lower=-0.3, upper=torch.tensor([0.3, 0.25, 1.0], device=dev), reg=1e-6, damping=2e-3,
              init=torch.tensor([[0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [-0.2, 0.1, 0.0]], device=dev))
    reg = _register(chain, observed, information, cells, reach, **kw)
    rounds = kw.pop("rounds")
    _same_registration(reg, *_loop(chain, observed, information, cells, reach, rounds, kw.pop("iterations"), **kw))
    assert reg.commands_history.shape == (4, m, 3) and reg.cost_history.dtype == torch.float64 and reg.found_history.dtype == torch.int32
    assert reg.fit.moments.shape == (m, 3, 74) and (reg.found_history > 0).all()
    assert torch.equal(reg.commands_history[-1], reg.fit.commands) and torch.equal(reg.found_history[-1], reg.matches.found)
    assert (reg.fit.commands <= torch.tensor([0.3, 0.25, 1.0], device=dev)).all() and (reg.fit.commands >= -0.3).all()


@pytest.mark.parametrize("angles", [(0.1, 0.1), (0.2, -0.2), (-0.3, 0.3)])
def test_planted_hinge_angles_are_recovered_with_planes_and_with_the_identity(dev, chain, angles):
    from neural_jacobian_field_amd.field_volume import cloud_registration_metric, plane_information, ray_information
    planted = np.float32([[angles[0] / 0.7, angles[1] / 1.3, 0.0]])
    observed, normals = _observation(chain, planted, np.random.default_rng(1), surface=True)
    observed, normals = _t(dev, observed[0]), _t(dev, normals[0])
    cells, reach = _scene_cells(chain.scene), 4 * chain.scene["step"][0]
    for name, information in (("planes", plane_information(normals)), ("identity", ray_information(normals, 1.0))):
        reg = _register(chain, observed, information, cells, reach, rounds=12, iterations=3)
        err = np.abs(_np(reg.fit.commands) - planted).max()
        print(f"{name}, angles {angles}: |u - planted| {err:.2e}, cost {reg.fit.cost.tolist()}, found {reg.found_history[:, 0].tolist()}")
        assert err <= RECOVERY and not reg.fit.status.any()
    cloud = _cloud(chain)
    again = cloud_registration_metric(cloud, _t(dev, chain.labels), chain.tw, observed, information, reach, cells=cells, joints=chain.joints,
                                      tree=chain.tree, rounds=12, iterations=3)
    for f in OUTPUTS:
        assert torch.equal(_bytes(getattr(again.fit, f)), _bytes(getattr(reg.fit, f))), f
