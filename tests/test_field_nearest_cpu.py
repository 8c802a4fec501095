"""Host-side tests of the closest-point query and the registration loop (field_volume.cell_grid / nearest_points /
register_commands / cloud_registration; njf_field_nearest): the numpy restatement
(tests/field_nearest_restatement.py) -- the ring search with its stop rule against the brute-force definition, exactly; the
registration loop on the planted chain, with a full, a partial and padded observation and from several starts -- and every
argument check, raised before any device work: there is no GPU here; the C ABI's symbol and return codes.

Recovery is held to 1e-5, the bound of the handle tests of section 18: the observed cloud holds the posed rows themselves, so
at the planted command every matched distance is 0 and the solver's minimum is the planted command up to the fp32 lattice of
the iterate (6e-8 at 1)."""
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_commands_restatement as F
import field_joints_restatement as J
import field_nearest_restatement as N
import field_pose_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 20
RECOVERY = 1e-5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


# ---- the stop rule ------------------------------------------------------------------------------------------------------------------
def _random_case(rng, kind):
    """A lattice, points and queries: kind 0 generic, 1 lattice-aligned on half cells (ties), 2 degenerate dims / one cell."""
    dims = tuple(int(d) for d in rng.integers(1, 9, 3))
    if kind == 2:
        dims = tuple(1 if rng.random() < 0.6 else d for d in dims)
    cell = np.float32(rng.uniform(0.05, 0.5))
    origin = rng.uniform(-1, 1, 3).astype(np.float32)
    extent = np.asarray(dims) * cell
    mo, mq = [(1, 1), (1, 3), (3, 1), (2, 2)][int(rng.integers(0, 4))]
    t, n = int(rng.integers(1, 120)), int(rng.integers(1, 60))

    def cloud(sets, rows, outside):
        u = rng.uniform(-outside, 1 + outside, (sets, rows, 3))
        if kind == 1:
            u = np.round(u * np.asarray(dims) * 2) / (np.asarray(dims) * 2)
        return (origin + u * extent).astype(np.float32)

    observed, queries = cloud(mo, t, 0.4), cloud(mq, n, 0.6)
    if kind == 2 and rng.random() < 0.5:                       # all points in one cell
        observed = (origin + (0.25 + 0.5 * rng.random((mo, t, 3))) * cell).astype(np.float32)
    bad = rng.random((mo, t)) < 0.1
    observed[bad, int(rng.integers(0, 3))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
    queries[rng.random((mq, n)) < 0.05, 0] = np.nan
    observed_count = None if rng.random() < 0.5 else rng.integers(0, t + 3, mo).astype(np.int32)
    count = None if rng.random() < 0.5 else int(rng.integers(0, n + 2))
    labels = None if rng.random() < 0.5 else rng.integers(-1, 3, n).astype(np.int32)
    reach = float(cell) * float(rng.choice([0.3, 1.0, 2.5, 6.0, 40.0]))
    return dict(observed=observed, queries=queries, origin=origin, cell=cell, dims=dims, max_distance=reach,
                observed_count=observed_count, count=count, labels=labels)


def _same(a, b, fields=("index", "distance2", "matched", "found")):
    for f in fields:
        x, y = np.asarray(a[f]), np.asarray(b[f])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f


def test_the_ring_search_is_the_brute_force_arg_min():
    rng = np.random.default_rng(19)
    stops, searched, found = np.zeros(N.MAX_RINGS + 1, np.int64), 0, 0
    for case in range(45):
        c = _random_case(rng, case % 3)
        want = N.brute(c["observed"], c["queries"], c["max_distance"], c["observed_count"], c["count"], c["labels"])
        got = N.rings(**c)
        _same(got, want)
        rows = got["rings"] >= 0
        stops += np.bincount(got["rings"][rows], minlength=N.MAX_RINGS + 1)
        searched, found = searched + int(rows.sum()), found + int(want["found"].sum())
        # rows outside the search are written, and with nothing
        assert (want["index"][~rows] == -1).all() and np.isinf(want["distance2"][~rows]).all() and np.isnan(want["matched"][~rows]).all()
    print(f"ring search: {searched} searched rows, {found} found; stopped after ring {dict(enumerate(stops.tolist())) }")
    assert searched > 1500 and found > 500 and stops[0] > 0 and stops[1] > 0 and stops[3:].sum() > 0


def test_ties_go_to_the_lowest_index_and_the_distance_is_inclusive():
    pts = np.float32([[0, 0, 0], [2, 0, 0], [2, 0, 0], [0, 2, 0], [np.nan, 0, 0], [1, 1, 7]])
    q = np.float32([[1, 0, 0], [2, 0, 0], [0.5, 0, 3], [np.inf, 0, 0]])
    for search in (lambda **kw: N.brute(pts, q, **kw), lambda **kw: N.rings(pts, q, (-1, -1, -1), 0.75, (4, 4, 2), **kw)):
        out = search(max_distance=1.0)
        assert out["index"].tolist() == [[0, 1, -1, -1]] and out["found"].tolist() == [2]
        assert out["distance2"].tolist() == [[1.0, 0.0, np.inf, np.inf]] and np.isnan(out["matched"][0, 2:]).all()
        assert out["matched"][0, :2].tolist() == [[0, 0, 0], [2, 0, 0]]
        assert search(max_distance=0.999)["index"].tolist() == [[-1, 1, -1, -1]]
        assert search(max_distance=1.0, observed_count=np.int32([1]))["index"].tolist() == [[0, -1, -1, -1]]
        assert search(max_distance=1.0, count=1, labels=np.int32([-1, 0, 0, 0]))["found"].tolist() == [0]
        assert search(max_distance=30.0)["index"].tolist() == [[0, 1, 0, -1]]


# ---- the registration loop on the planted chain ------------------------------------------------------------------------------------
def _chain_scene():
    chain = J.chain()
    ref = J.run(chain)
    tree = (np.array([-1, 0, 1], np.int32), np.array([-1, 0, 1], np.int32))
    xyz = J.node_coordinates(chain["dims"], chain["index"]).astype(np.float32)
    return dict(scene=chain, twists=R.twists_of(chain), joints=R.joints_of(ref), tree=tree, xyz=xyz, labels=chain["labels"],
                parts=chain["parts"], step=float(J.STEP[0]))


@pytest.fixture(scope="module")
def chain():
    return _chain_scene()


def planted_command(angles):
    """The chain's command of hinge angles (rad) on its two hinges: the twists turn by 0.7 and 1.3 rad per unit command."""
    return np.float32([[angles[0] / 0.7, angles[1] / 1.3, 0.0]])


def observation(s, command, seed, keep=None, nans=0):
    """The rows posed at ``command`` in shuffled order, optionally only the rows ``keep`` and with NaN rows mixed in."""
    rng = np.random.default_rng(seed)
    posed = F.posed_targets(s["twists"], command, s["xyz"], s["labels"], s["parts"], s["joints"], s["tree"])[0]
    if keep is not None:
        posed = posed[keep]
    posed = np.concatenate([posed, np.full((nans, 3), np.nan, np.float32)])
    return posed[rng.permutation(posed.shape[0])]


def _register(s, observed, reach, **kw):
    return N.register(s["twists"], s["xyz"], s["labels"], observed, reach, s["parts"], s["joints"], s["tree"], **kw)


@pytest.mark.parametrize("angles", [(0.1, 0.1), (0.2, -0.2), (-0.3, 0.3), (0.3, 0.3)])
def test_a_planted_command_is_recovered_from_a_shuffled_cloud(chain, angles):
    assert chain["xyz"].shape[0] == 272
    planted = planted_command(angles)
    out = _register(chain, observation(chain, planted, seed=1), 4 * chain["step"], rounds=12, iterations=3)
    err = np.abs(out["fit"]["commands"] - planted).max()
    print(f"angles {angles}: |u - planted| {err:.2e}, cost {out['fit']['cost'][0]:.2e}, found {out['found_history'][:, 0].tolist()}")
    assert err <= RECOVERY
    assert out["commands_history"].shape == (12, 1, 3) and out["cost_history"].shape == (12, 1) and out["found_history"].shape == (12, 1)
    assert out["commands_history"][-1].tobytes() == out["fit"]["commands"].tobytes()


@pytest.mark.parametrize("cells", (2, 4))
@pytest.mark.parametrize("angle", (0.2, 0.3))
def test_a_partial_padded_observation_recovers_the_command(chain, angle, cells):
    planted = planted_command((angle, -angle))
    links = np.flatnonzero(chain["labels"] != chain["parts"][0])            # the base part is not observed
    observed = observation(chain, planted, seed=2, keep=links, nans=17)
    out = _register(chain, observed, cells * chain["step"], rounds=8, iterations=3)
    err = np.abs(out["fit"]["commands"] - planted).max()
    print(f"partial, {angle} rad, reach {cells} steps: |u - planted| {err:.2e}, found {out['found_history'][:, 0].tolist()}")
    assert err <= RECOVERY
    assert (out["found_history"] < chain["xyz"].shape[0]).all() and out["found_history"][-1, 0] > 0


def test_several_starts_against_one_observation(chain):
    planted = planted_command((0.45, 0.6))
    observed = observation(chain, planted, seed=3)
    starts = np.float32([[a / 0.7, b / 1.3, 0.0] for a in (-0.6, 0.0, 0.6) for b in (-0.35, 0.0, 0.35)])
    out = _register(chain, observed[None], 4 * chain["step"], init=starts, rounds=12, iterations=3)
    cost = out["fit"]["cost"]
    best = int(cost.argmin())
    err = np.abs(out["fit"]["commands"] - planted).max(axis=1)
    print(f"nine starts: costs {cost}, errors {err}, best {best}")
    assert cost.shape == (9,) and err[best] <= RECOVERY


# ---- argument errors ------------------------------------------------------------------------------------------------------------------
def _cpu_arguments():
    chain = J.chain()
    tw = J.field_twists(chain)
    joints = J.field_joints(chain, J.run(chain), tw)
    n = chain["labels"].shape[0]
    return tw, joints, joints.tree(), torch.zeros(n, 3), torch.from_numpy(chain["labels"]), torch.zeros(2, 50, 3)


def test_cell_grid():
    from neural_jacobian_field_amd.field_volume import FieldGrid, cell_grid
    g = cell_grid((-1.0, 0.0, 2.0), (1.0, 0.05, 2.0), 0.1)
    assert isinstance(g, FieldGrid) and g.dims == (20, 1, 1) and g.origin == (-1.0, 0.0, 2.0)
    assert g.step == (float(np.float32(0.1)),) * 3
    assert cell_grid((0, 0, 0), (1, 1, 1), 0.3).dims == (4, 4, 4)
    assert cell_grid((0, 0, 0), (1024, 1, 1), 1).dims == (1024, 1, 1)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="cell_grid: cell must be"):
            cell_grid((0, 0, 0), (1, 1, 1), bad)
    for lo, hi in (((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, float("inf"))), (None, (1, 1, 1)), ((0, 0, "x"), (1, 1, 1))):
        with pytest.raises(ValueError, match="cell_grid: lower and upper have three"):
            cell_grid(lo, hi, 0.1)
    with pytest.raises(ValueError, match="cell_grid: lower > upper"):
        cell_grid((0, 2, 0), (1, 1, 1), 0.1)
    with pytest.raises(ValueError, match="cell_grid: at most 1024 cells per axis"):
        cell_grid((0, 0, 0), (1, 1025, 1), 1.0)


def test_nearest_points_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, cell_grid, nearest_points
    q, obs = torch.zeros(2, 40, 3), torch.zeros(2, 50, 3)
    cells = cell_grid((0, 0, 0), (1, 1, 1), 0.1)
    for bad in (q.double(), q[..., :2], q[0, 0], None, np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="nearest_points: queries must be fp32"):
            nearest_points(bad, obs, cells, 0.1)
    for bad in (obs.double(), obs[..., :2], obs[0, 0], None, torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError, match="nearest_points: observed must be fp32"):
            nearest_points(q, bad, cells, 0.1)
    with pytest.raises(ValueError, match="nearest_points: observed and queries hold one set or one per problem"):
        nearest_points(q, torch.zeros(3, 50, 3), cells, 0.1)
    with pytest.raises(ValueError, match="nearest_points: 1 to 65535 problems"):
        nearest_points(torch.zeros(0, 40, 3), obs[:1], cells, 0.1)
    with pytest.raises(ValueError, match="nearest_points: 1 to 65535 problems"):
        nearest_points(torch.zeros(65536, 1, 3), obs[:1], cells, 0.1)
    for bad in (None, (0, 0, 0), cells.c_grid()):
        with pytest.raises(ValueError, match="nearest_points: cells must be a FieldGrid"):
            nearest_points(q, obs, bad, 0.1)
    for bad in (FieldGrid((0, 0, 0), (0.1, 0.1, 0.2), (4, 4, 4)), FieldGrid((0, 0, 0), (0.0, 0.0, 0.0), (4, 4, 4)),
                FieldGrid((0, 0, 0), (-0.1, -0.1, -0.1), (4, 4, 4))):
        with pytest.raises(ValueError, match="nearest_points: cells must have three equal steps > 0"):
            nearest_points(q, obs, bad, 0.1)
    with pytest.raises(ValueError, match="nearest_points: at most 1024 cells per axis"):
        nearest_points(q, obs, FieldGrid((0, 0, 0), (0.1, 0.1, 0.1), (1025, 1, 1)), 0.1)
    with pytest.raises(ValueError, match="nearest_points: Mo \\* the number of cells"):
        nearest_points(q, obs, FieldGrid((0, 0, 0), (0.1, 0.1, 0.1), (1024, 1024, 1024)), 0.1)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, "1", None, True):
        with pytest.raises(ValueError, match="nearest_points: max_distance must be a finite number > 0"):
            nearest_points(q, obs, cells, bad)
    nearest = float(np.float32(0.1))
    for bad in (63.001 * nearest, 100.0, 1e30, 1e39):
        with pytest.raises(ValueError, match="nearest_points: max_distance may span at most 63 cells"):
            nearest_points(q, obs, cells, bad)
    for bad in (3, torch.ones(3, dtype=torch.int32), torch.ones(2), torch.ones(2, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="nearest_points: observed_count must be int32 \\[2\\]"):
            nearest_points(q, obs, cells, 0.1, observed_count=bad)
    for bad in (3, torch.ones(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="nearest_points: count must be one int32"):
            nearest_points(q, obs, cells, 0.1, count=bad)
    for bad in (torch.zeros(40), torch.zeros(39, dtype=torch.int32), [0] * 40):
        with pytest.raises(ValueError, match="nearest_points: labels must be int32 \\[40\\]"):
            nearest_points(q, obs, cells, 0.1, labels=bad)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="nearest_points: observed must live on the device of queries"):
            nearest_points(q.cuda(), obs, cells, 0.1)
    for args, kw in (((q, obs), {}), ((q[0], obs[0]), {}), ((q, obs[0]), {}), ((q[0], obs), {}),
                     ((q, obs), dict(observed_count=torch.ones(2, dtype=torch.int32), count=torch.ones(1, dtype=torch.int32),
                                     labels=torch.zeros(40, dtype=torch.int32)))):
        with pytest.raises(ValueError, match="nearest_points: .*no CPU path"):
            nearest_points(*args, cells, 6.0, **kw)


def test_register_commands_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import cell_grid, register_commands
    tw, joints, tree, xyz, labels, obs = _cpu_arguments()
    n = xyz.shape[0]
    cells = cell_grid((0, 0, 0), (1, 1, 1), 0.1)
    go = lambda *a, **kw: register_commands(*a, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="register_commands: twists must be a FieldTwists"):
        go(None, xyz, labels, obs, cells, 0.1)
    with pytest.raises(ValueError, match="register_commands: xyz must be fp32"):
        go(tw, xyz.double(), labels, obs, cells, 0.1)
    with pytest.raises(ValueError, match="register_commands: labels must be int32"):
        go(tw, xyz, labels.long(), obs, cells, 0.1)
    for bad in (0, 1001, 2.0, True, None):
        with pytest.raises(ValueError, match="register_commands: rounds must be an integer in \\[1, 1000\\]"):
            go(tw, xyz, labels, obs, cells, 0.1, rounds=bad)
    with pytest.raises(ValueError, match="register_commands: observed must be fp32"):
        go(tw, xyz, labels, obs.double(), cells, 0.1)
    with pytest.raises(ValueError, match="register_commands: cells must be a FieldGrid"):
        go(tw, xyz, labels, obs, None, 0.1)
    with pytest.raises(ValueError, match="register_commands: max_distance must be"):
        go(tw, xyz, labels, obs, cells, 0.0)
    with pytest.raises(ValueError, match="register_commands: max_distance may span at most 63 cells"):
        go(tw, xyz, labels, obs, cells, 7.0)
    with pytest.raises(ValueError, match="register_commands: observed_count must be int32 \\[2\\]"):
        go(tw, xyz, labels, obs, cells, 0.1, observed_count=torch.ones(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="register_commands: observed and queries hold one set or one per problem"):
        go(tw, xyz, labels, obs, cells, 0.1, init=torch.zeros(3, 3))
    for bad in (torch.zeros(3), torch.zeros(2, 3).double(), torch.zeros(2, 4)):
        with pytest.raises(ValueError, match="register_commands: init must be fp32 \\[2, 3\\]"):
            go(tw, xyz, labels, obs, cells, 0.1, init=bad)
    with pytest.raises(ValueError, match="register_commands: weights must be fp32"):
        go(tw, xyz, labels, obs, cells, 0.1, weights=torch.ones(n - 1))
    with pytest.raises(ValueError, match="register_commands: lower must be fp32"):
        go(tw, xyz, labels, obs, cells, 0.1, lower=torch.zeros(2))
    with pytest.raises(ValueError, match="register_commands: lower > upper"):
        go(tw, xyz, labels, obs, cells, 0.1, lower=0.5, upper=-0.5)
    with pytest.raises(ValueError, match="register_commands: reg must be"):
        go(tw, xyz, labels, obs, cells, 0.1, reg=-1.0)
    with pytest.raises(ValueError, match="register_commands: damping must be"):
        go(tw, xyz, labels, obs, cells, 0.1, damping=0.0)
    with pytest.raises(ValueError, match="register_commands: iterations must be an integer"):
        go(tw, xyz, labels, obs, cells, 0.1, iterations=1001)
    with pytest.raises(ValueError, match="register_commands: joints and tree come together"):
        go(tw, xyz, labels, obs, cells, 0.1, joints=joints)
    with pytest.raises(ValueError, match="register_commands: tree (parent|joint_of) must be int32"):
        go(tw, xyz, labels, obs, cells, 0.1, joints=joints, tree=joints.parents())
    with pytest.raises(ValueError, match="register_commands: count must be one int32"):
        go(tw, xyz, labels, obs, cells, 0.1, count=3)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="register_commands: observed must live on the device of xyz"):
            go(tw, xyz, labels, obs.cuda(), cells, 0.1)
    for o, kw in ((obs, {}), (obs[0], {}), (obs[:1], dict(init=torch.zeros(9, 3), joints=joints, tree=tree, lower=-1.0, upper=torch.ones(3),
                                                           weights=torch.ones(n), rounds=1000, iterations=0, reg=0.5,
                                                           observed_count=torch.ones(1, dtype=torch.int32),
                                                           count=torch.tensor([n], dtype=torch.int32)))):
        with pytest.raises(ValueError, match="register_commands: .*no CPU path"):
            go(tw, xyz, labels, o, cells, 0.1, **kw)


def test_cloud_registration_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud, cell_grid, cloud_registration
    tw, joints, tree, xyz, labels, obs = _cpu_arguments()
    chain = J.chain()
    n = xyz.shape[0]
    cloud = FieldPointCloud(grid=FieldGrid(chain["origin"], chain["step"], chain["dims"]), index=torch.from_numpy(chain["index"]),
                            xyz=xyz, density=torch.ones(n), color=None, jacobian=None, count=torch.tensor([n], dtype=torch.int32))
    with pytest.raises(ValueError, match="cloud_registration: cloud must be a FieldPointCloud"):
        cloud_registration(None, labels, tw, obs, 0.1)
    with pytest.raises(ValueError, match="cloud_registration: labels must be int32"):
        cloud_registration(cloud, labels.long(), tw, obs, 0.1)
    with pytest.raises(ValueError, match="cloud_registration: observed must be fp32"):
        cloud_registration(cloud, labels, tw, obs[0, 0], 0.1)
    with pytest.raises(ValueError, match="cloud_registration: count must be one int32"):
        cloud_registration(dataclasses.replace(cloud, count=torch.ones(2, dtype=torch.int32)), labels, tw, obs, 0.1)
    with pytest.raises(ValueError, match="cloud_registration: rounds must be"):
        cloud_registration(cloud, labels, tw, obs, 0.1, rounds=0)
    with pytest.raises(ValueError, match="cloud_registration: max_distance may span at most 63 cells"):
        cloud_registration(cloud, labels, tw, obs, 64.0 * max(chain["step"]))              # (the default cells: the grid's step)
    with pytest.raises(ValueError, match="cloud_registration: cell must be"):
        cloud_registration(dataclasses.replace(cloud, grid=FieldGrid((0, 0, 0), (0, 0, 0), (1, 1, 1))), labels, tw, obs, 0.1)
    for kw in ({}, dict(cells=cell_grid((0, 0, 0), (1, 1, 1), 0.25), joints=joints, tree=tree)):
        with pytest.raises(ValueError, match="cloud_registration: .*no CPU path"):
            cloud_registration(cloud, labels, tw, obs, 0.1, **kw)


def test_the_signatures():
    from neural_jacobian_field_amd import field_volume as fv
    params = inspect.signature(fv.cell_grid).parameters
    assert list(params) == ["lower", "upper", "cell"]
    keywords = dict(observed_count=None, count=None, labels=None)
    params = inspect.signature(fv.nearest_points).parameters
    assert list(params) == ["queries", "observed", "cells", "max_distance"] + list(keywords)
    assert {k: params[k].default for k in keywords} == keywords
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    keywords = dict(joints=None, tree=None, observed_count=None, count=None, weights=None, init=None, lower=None, upper=None, reg=0.0,
                    rounds=8, iterations=3, damping=1e-3)
    params = inspect.signature(fv.register_commands).parameters
    assert list(params) == ["twists", "xyz", "labels", "observed", "cells", "max_distance"] + list(keywords)
    assert {k: params[k].default for k in keywords} == keywords
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    params = inspect.signature(fv.cloud_registration).parameters
    del keywords["count"]
    keywords = dict(cells=None, **keywords)
    assert list(params) == ["cloud", "labels", "twists", "observed", "max_distance"] + list(keywords)
    assert {k: params[k].default for k in keywords} == keywords
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    assert list(fv.FieldNearest.__dataclass_fields__) == ["index", "distance2", "matched", "found"]
    assert list(fv.FieldRegistration.__dataclass_fields__) == ["fit", "matches", "commands_history", "cost_history", "found_history"]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "njf_field_nearest" in declared and "njf_field_nearest" in hip.EXPORTED_SYMBOLS and hasattr(lib, "njf_field_nearest")
    params = re.search(r"njf_field_nearest\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_nearest.argtypes) == ARGUMENTS
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_NEAREST_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_NEAREST_ALL"] == hip.FIELD_NEAREST_ALL == sum(hip.FIELD_NEAREST_PHASES)
    assert [defines[f"NJF_FIELD_NEAREST_{n.upper()}"] for n in hip.FIELD_NEAREST_PHASE_NAMES] == list(hip.FIELD_NEAREST_PHASES)
    assert defines["NJF_FIELD_NEAREST_WAVE"] == hip.FIELD_NEAREST_WAVE == 4
    assert defines["NJF_FIELD_NEAREST_MAX_RINGS"] == hip.FIELD_NEAREST_MAX_RINGS == N.MAX_RINGS == 64
    assert defines["NJF_FIELD_NEAREST_MAX_DIM"] == hip.FIELD_NEAREST_MAX_DIM == N.MAX_DIM == 1024
    assert "NJF_FIELD_NEAREST_WORKSPACE(Mo, C, T)" in header
    assert hip.field_nearest_workspace(3, 1000, 77) == 3 * 1001 + 3 * 1000 + 4 * 3 * 77 + 3
    assert hip.field_nearest_workspace(1, 1, 1) == 2 + 1 + 4 + 3


def test_the_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("observed", "observed_count", "num_observed", "points", "queries", "count", "labels", "num_queries", "n", "num_problems",
             "cells", "max_distance", "index", "distance2", "matched", "found", "workspace", "workspace_words", "phases")
    assert len(names) + 1 == ARGUMENTS
    need = hip.field_nearest_workspace(5, 8 * 9 * 10, 5000)

    def call(origin=(0.0, 0.0, 0.0), step=(0.25, 0.25, 0.25), dims=(8, 9, 10), **kw):
        args = {k: P for k in names}
        args.update(num_observed=5, points=5000, num_queries=5, n=300, num_problems=5, max_distance=0.5, workspace_words=need, phases=3,
                    cells=hip.make_field_grid(origin, step, dims))
        args.update(kw)
        return lib.njf_field_nearest(*[args[k] for k in names], None)

    for key, values in (("num_problems", (0, -1, 65536)), ("num_observed", (0, 2, 6)), ("num_queries", (0, 4, -5)),
                        ("phases", (0, -1, 4, 5, 8)), ("max_distance", (0.0, -1.0, float("nan"), float("inf"), 1e-60, 15.76, 1e39))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)
    for dims in ((0, 9, 10), (8, -1, 10), (8, 9, 1025)):
        assert call(dims=dims) == E_VALUE
    for step in ((0.25, 0.25, 0.5), (0.0, 0.0, 0.0), (-0.25,) * 3, (float("nan"),) * 3, (float("inf"),) * 3, (1e-45,) * 3):
        assert call(step=step) == E_VALUE, step
    assert call(origin=(0.0, float("nan"), 0.0)) == E_VALUE
    assert call(dims=(1024, 1024, 512), workspace_words=2 ** 62) == E_VALUE               # 5 * 2^29 cells
    assert call(dims=(1024, 1024, 1024), num_observed=1, workspace_words=2 ** 62, workspace=None) == E_NULL   # 2^30 cells pass
    assert call(n=-1) == E_SHAPE
    assert call(points=0) == E_SHAPE
    assert call(points=2 ** 29, workspace_words=2 ** 62) == E_SHAPE                      # Mo * T = 5 * 2^29
    assert call(workspace_words=need - 1) == E_SHAPE
    for key in ("observed", "queries", "cells", "index", "distance2", "matched", "found", "workspace"):
        assert call(**{key: None}) == E_NULL, key
    # the build needs no query and no output, the query no observed points
    assert call(phases=2, found=None) == E_NULL and call(phases=1, observed=None) == E_NULL
    assert call(phases=6, queries=None) == E_NULL and call(phases=7, matched=None) == E_NULL
    assert call(max_distance=15.75, found=None) == E_NULL                                 # 63 cells: the last permitted reach
