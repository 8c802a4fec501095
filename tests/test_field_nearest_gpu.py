"""GPU tests of the closest-point query and the registration loop (field_volume.nearest_points / register_commands /
cloud_registration; njf_field_nearest) against the numpy restatement of their semantics
(tests/field_nearest_restatement.py).

The query is held to the brute-force definition EXACTLY, in all four outputs and in both forms of the query launch: the
arg-min of an fp32 expression with a lowest-index tie-break has one answer.  The registration is held byte for byte to a loop
written here from the public pieces, and to the recovery bound of the host-side tests (1e-5).

Run with -m gpu."""
import numpy as np
import pytest
import torch

import block_offsets_cases as K
import field_commands_restatement as F
import field_joints_restatement as J
import field_nearest_restatement as N
import field_pose_restatement as R
from test_field_commands_gpu import Scene, _line

pytestmark = pytest.mark.gpu

IMG = 64
RECOVERY = 1e-5
NEAR = ("index", "distance2", "matched", "found")
FIT = ("commands", "cost", "initial_cost", "weight", "steps", "gradient", "status", "part_status", "depth", "moments")
HISTORY = ("commands_history", "cost_history", "found_history")


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
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _cells(origin, cell, dims):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid(tuple(float(v) for v in origin), (float(cell),) * 3, tuple(int(d) for d in dims))


def _scene_cells(scene):
    from neural_jacobian_field_amd.field_volume import cell_grid
    upper = [o + s * (d - 1) for o, s, d in zip(scene["origin"], scene["step"], scene["dims"])]
    return cell_grid(scene["origin"], upper, max(scene["step"]))


def _raw(dev, observed, queries, cells, reach, phase, m, observed_count=None, count=None, labels=None, fill=None):
    """hip.field_nearest on outputs of the test's own, optionally sentinel-filled; a dict of tensors."""
    from neural_jacobian_field_amd import hip
    n = queries.shape[1]
    out = dict(index=torch.empty(m, n, dtype=torch.int32, device=dev), distance2=torch.empty(m, n, device=dev),
               matched=torch.empty(m, n, 3, device=dev), found=torch.empty(m, dtype=torch.int32, device=dev))
    if fill is not None:
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
    hip.field_nearest(observed, queries, cells.c_grid(), reach, out, m, observed_count=observed_count, count=count, labels=labels,
                      phase=phase)
    return out


def _check(dev, observed, queries, cells, reach, observed_count=None, count=None, labels=None, what=""):
    """The device, in both forms of the query launch, against the brute-force restatement: equal bytes in all four outputs."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import nearest_points
    want = N.brute(observed, queries, reach, observed_count, count, labels)
    kw = dict(observed_count=_t(dev, observed_count), count=None if count is None else torch.tensor([count], dtype=torch.int32, device=dev),
              labels=_t(dev, labels))
    got = nearest_points(_t(dev, queries), _t(dev, observed), cells, reach, **kw)
    o3, q3 = (_t(dev, v if v.ndim == 3 else v[None]) for v in (observed, queries))
    wave = _raw(dev, o3, q3, cells, reach, hip.FIELD_NEAREST_ALL | hip.FIELD_NEAREST_WAVE, want["index"].shape[0], fill=0x5a, **kw)
    for f in NEAR:
        lane = _np(getattr(got, f))
        assert lane.dtype == want[f].dtype and lane.shape == want[f].shape, f
        differ = int((lane.view(np.uint8) != want[f].view(np.uint8)).sum())
        assert differ == 0, (what, f, differ)
        assert _np(wave[f]).tobytes() == want[f].tobytes(), (what, f, "wave")
    print(f"{what}: {want['index'].size} rows, found {want['found'].tolist()}")
    return got, want


def _cloud(rng, sets, rows, origin, extent, outside):
    return (np.asarray(origin) + rng.uniform(-outside, 1 + outside, (sets, rows, 3)) * np.asarray(extent)).astype(np.float32)


# ---- (a) the query against the definition ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(dev):
    return Scene(dev, J.chain())


@pytest.mark.parametrize("mo,mq", ((1, 1), (3, 3), (1, 3), (3, 1)))
def test_the_chain_against_its_shuffled_posed_rows(dev, chain, mo, mq):
    rng = np.random.default_rng(21)
    u = np.float32([[0.2, -0.1, 0.0], [-0.3, 0.2, 0.5], [0.05, 0.3, -1.0]])
    posed = chain.targets(u)
    observed = np.stack([posed[i][rng.permutation(posed.shape[1])] for i in range(mo)])
    queries = np.stack([chain.xyz] * mq) if mq == 1 else chain.targets(0.5 * u)
    got, want = _check(dev, observed, queries, _scene_cells(chain.scene), 4 * chain.scene["step"][0], what=f"chain Mo {mo} Mq {mq}")
    assert want["index"].shape == (max(mo, mq), 272) and want["found"].min() > 100


@pytest.mark.parametrize("n,t,dims", ((257, 300, (5, 4, 3)), (4097, 1000, (7, 8, 6)), (63, 1, (3, 3, 3)), (300, 500, (1, 1, 1)),
                                      (500, 700, (12, 1, 9))))
def test_random_clouds_inside_and_outside_the_box(dev, n, t, dims):
    rng = np.random.default_rng(n + t)
    cell, origin = 0.11, (-0.4, 0.3, 1.0)
    extent = np.asarray(dims) * cell
    observed, queries = _cloud(rng, 2, t, origin, extent, 0.4), _cloud(rng, 2, n, origin, extent, 0.6)
    observed[rng.random((2, t)) < 0.05, 1] = np.nan
    observed[rng.random((2, t)) < 0.03, 2] = np.inf
    queries[rng.random((2, n)) < 0.05, 0] = -np.inf
    queries[rng.random((2, n)) < 0.03, 2] = np.nan
    for reach in (0.9 * cell, 3.5 * cell):
        _check(dev, observed, queries, _cells(origin, cell, dims), reach, what=f"n {n} T {t} dims {dims} reach {reach:.3f}")


@pytest.mark.parametrize("dims,clouds", K.CELL_CASES)
def test_a_cell_list_past_256_scan_blocks(dev, dims, clouds):
    """The list's build with two sums per thread of the one-workgroup scan of its block sums (281 scan blocks of one cloud, 286 of
    three); the first queries sit at the centres of the cells at the seams of that scan, each with two points of its own
    (tests/block_offsets_cases.py, checked by tests/test_block_primitives_cpu.py)."""
    case = K.cell_case(dims, clouds)
    got, want = _check(dev, case["points"], case["queries"], _cells(K.CELL_ORIGIN, K.CELL_SIZE, dims), K.CELL_REACH,
                       what=f"cell list {dims} x {clouds}")
    blocks = K.workgroups(case["positions"], K.SCAN_BLOCK)
    print(f"scan blocks {blocks}, per {K.per_thread(blocks)}, found {want['found'].tolist()} of {K.CELL_QUERIES}")
    assert blocks > K.THREADS and want["found"].min() > K.CELL_QUERIES // 2
    crafted = {(cloud, row) for cloud, row, _ in case["crafted"]}
    for cloud in range(clouds):
        seams = sum(p // case["cells"] == cloud for p in K.crafted_positions(dims, clouds))
        assert all((cloud, int(j)) in crafted for j in want["index"][cloud, :seams])


def test_one_crowded_cell_and_ties(dev):
    rng = np.random.default_rng(5)
    cell, origin, dims = 0.25, (0.0, 0.0, 0.0), (4, 4, 4)
    crowd = (np.float32([0.3, 0.3, 0.3]) + 0.2 * rng.random((1, 300, 3))).astype(np.float32)              # 300 points in cell (1, 1, 1)
    queries = _cloud(rng, 1, 200, origin, (1, 1, 1), 0.3)
    _check(dev, crowd, queries, _cells(origin, cell, dims), 1.0, what="one crowded cell")
    # lattice-aligned points, each several times over: the lowest index wins, in two insertion orders of the same set
    nodes = np.stack(np.meshgrid(*[np.arange(5) * 0.25] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    points = np.concatenate([nodes, nodes[::2], nodes[::3]])
    half = (rng.integers(0, 9, (1, 400, 3)) * 0.125).astype(np.float32)                                   # on half-cell positions
    for order in (np.arange(points.shape[0]), rng.permutation(points.shape[0])):
        got, want = _check(dev, points[order][None], half, _cells(origin, cell, dims), 0.5, what="ties")
        first = {tuple(p): j for j, p in reversed(list(enumerate(points[order].tolist())))}              # the lowest index of every point
        index, matched = want["index"][0], want["matched"][0]
        assert all(first[tuple(matched[i].tolist())] == index[i] for i in range(400) if index[i] >= 0) and (index >= 0).sum() > 300


def test_counts_labels_and_rows_that_are_not_read(dev):
    rng = np.random.default_rng(8)
    cell, origin, dims = 0.2, (-1.0, -1.0, -1.0), (10, 10, 10)
    observed, queries = _cloud(rng, 3, 400, origin, (2, 2, 2), 0.1), _cloud(rng, 3, 333, origin, (2, 2, 2), 0.1)
    queries[:, 300:] = np.float32([np.nan, 3e38, -np.inf])                                                # garbage behind the count
    labels = rng.integers(-2, 4, 333).astype(np.int32)
    got, want = _check(dev, observed, queries, _cells(origin, cell, dims), 0.35, observed_count=np.int32([0, 9999, 123]), count=300,
                       labels=labels, what="counts and labels")
    assert want["found"][0] == 0 and (want["index"][0] == -1).all() and want["found"][1] > 0
    assert (want["index"][:, 300:] == -1).all() and (want["index"][:, labels < 0] == -1).all() and want["index"][2].max() < 123
    _check(dev, observed, queries, _cells(origin, cell, dims), 0.35, observed_count=np.int32([-5, 1, 400]), count=9999, what="counts past the ends")


def test_nothing_within_reach_and_the_last_permitted_ring(dev):
    cell, origin, dims = 0.5, (0.0, 0.0, 0.0), (140, 2, 1)
    observed = np.float32([[[69.9, 0.25, 0.25], [31.6, 0.6, 0.1], [np.nan, 0, 0]]])
    queries = np.float32([[[0.1, 0.2, 0.3], [0.2, 0.7, 0.1], [38.4, 0.25, 0.25], [69.0, 0.9, 0.4], [-5.0, 0.5, 0.5]]])
    lattice = _cells(origin, cell, dims)
    got, want = _check(dev, observed, queries, lattice, 63 * cell, what="the last ring")                  # ceil(63) + 1 = 64 rings
    rings = N.rings(observed, queries, origin, cell, dims, 63 * cell)
    assert rings["rings"].max() == N.MAX_RINGS and want["index"].tolist() == [[-1, 1, 1, 0, -1]]
    for f in NEAR:
        assert rings[f].tobytes() == want[f].tobytes(), f
    got, want = _check(dev, observed, queries, lattice, 0.4, what="nothing within reach")
    assert want["found"].tolist() == [0] and (want["index"] == -1).all() and np.isnan(want["matched"]).all()


def test_a_line_of_256_parts_against_itself_posed(dev):
    s = _line(dev)
    assert s.xyz.shape[0] == 4352
    posed = s.targets((0.5 * np.random.default_rng(7).uniform(-1, 1, (2, 3))).astype(np.float32))
    from neural_jacobian_field_amd.field_volume import cell_grid
    cells = cell_grid(posed.reshape(-1, 3).min(axis=0).tolist(), posed.reshape(-1, 3).max(axis=0).tolist(), 0.05)
    got, want = _check(dev, posed[:, np.random.default_rng(3).permutation(4352)], s.xyz, cells, 0.2, what="line")
    assert want["found"].min() > 1000


# ---- (b) every row is written; determinism; capture -------------------------------------------------------------------------------------
def _case(dev, seed=31, m=3, t=900, n=1500):
    rng = np.random.default_rng(seed)
    cell, origin, dims = 0.1, (0.0, 0.0, 0.0), (9, 11, 7)
    observed, queries = _cloud(rng, m, t, origin, np.asarray(dims) * cell, 0.2), _cloud(rng, m, n, origin, np.asarray(dims) * cell, 0.3)
    queries[:, ::17, 1] = np.nan
    return observed, queries, _cells(origin, cell, dims), 0.23, np.int32([t, t // 2, 0][:m]), n - 100, rng.integers(-1, 3, n).astype(np.int32)


def test_sentinel_filled_outputs_are_written_and_two_calls_and_a_replay_agree(dev):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import nearest_points
    observed, queries, cells, reach, oc, count, labels = _case(dev)
    want = N.brute(observed, queries, reach, oc, count, labels)
    o, q = _t(dev, observed), _t(dev, queries)
    kw = dict(observed_count=_t(dev, oc), count=torch.tensor([count], dtype=torch.int32, device=dev), labels=_t(dev, labels))
    for fill in (0x00, 0xa5):
        out = _raw(dev, o, q, cells, reach, hip.FIELD_NEAREST_ALL, 3, fill=fill, **kw)
        for f in NEAR:
            assert _np(out[f]).tobytes() == want[f].tobytes(), (f, fill)
    first, second = (nearest_points(q, o, cells, reach, **kw) for _ in range(2))
    for f in NEAR:
        assert torch.equal(_bytes(getattr(first, f)), _bytes(getattr(second, f))), f
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        near = nearest_points(q, o, cells, reach, **kw)
    for f in NEAR:
        getattr(near, f).view(torch.uint8).fill_(0x77)
    graph.replay()
    torch.cuda.synchronize()
    for f in NEAR:
        assert torch.equal(_bytes(getattr(near, f)), _bytes(getattr(first, f))), f
    assert int(first.found.sum()) > 500


# ---- (c) the phases apart -----------------------------------------------------------------------------------------------------------------
def test_one_build_serves_two_queries(dev):
    from neural_jacobian_field_amd import hip
    observed, queries, cells, reach, oc, count, labels = _case(dev, seed=32, m=1)
    other = (queries[:, ::-1] + np.float32(0.013)).copy()
    o = _t(dev, observed)
    kw = dict(observed_count=_t(dev, oc), labels=_t(dev, labels))
    workspace = torch.empty(hip.field_nearest_workspace(1, cells.num_nodes, observed.shape[1]), dtype=torch.int32, device=dev)
    hip.field_nearest(o, (1, queries.shape[1]), cells.c_grid(), reach, None, 1, observed_count=kw["observed_count"],
                      phase=hip.FIELD_NEAREST_BUILD, workspace=workspace)
    for q in (queries, other):
        n = q.shape[1]
        out = dict(index=torch.empty(1, n, dtype=torch.int32, device=dev), distance2=torch.empty(1, n, device=dev),
                   matched=torch.empty(1, n, 3, device=dev), found=torch.empty(1, dtype=torch.int32, device=dev))
        hip.field_nearest(tuple(observed.shape[:2]), _t(dev, q), cells.c_grid(), reach, out, 1, phase=hip.FIELD_NEAREST_QUERY,
                          workspace=workspace, **kw)
        full = _raw(dev, o, _t(dev, q), cells, reach, hip.FIELD_NEAREST_ALL, 1, **kw)
        want = N.brute(observed, q, reach, oc, None, labels)
        for f in NEAR:
            assert torch.equal(_bytes(out[f]), _bytes(full[f])) and _np(out[f]).tobytes() == want[f].tobytes(), f


# ---- (d) the registration is its public pieces, and nothing else ----------------------------------------------------------------------------
def _loop(s, observed, cells, reach, rounds, iterations, init=None, lower=None, upper=None, observed_count=None, **kw):
    from neural_jacobian_field_amd.field_volume import nearest_points, part_poses, solve_commands
    dev = s.dev
    xyz, labels = _t(dev, s.xyz), _t(dev, s.labels)
    count = None if s.count is None else torch.tensor([s.count], dtype=torch.int32, device=dev)
    m = max(observed.shape[0] if observed.dim() == 3 else 1, 1 if init is None else init.shape[0])
    a_dim = s.twists["omega"].shape[1]
    u = torch.zeros(m, a_dim, device=dev) if init is None else init
    if lower is not None:
        u = torch.clamp(u, min=lower)
    if upper is not None:
        u = torch.clamp(u, max=upper)
    history = []
    for _ in range(rounds):
        posed = part_poses(s.tw, u, joints=s.joints, tree=s.tree).apply(xyz, labels, count=count)
        near = nearest_points(posed, observed, cells, reach, observed_count=observed_count, count=count, labels=labels)
        fit = solve_commands(s.tw, xyz, labels, near.matched, joints=s.joints, tree=s.tree, count=count, init=u, lower=lower, upper=upper,
                             iterations=iterations, **kw)
        history.append((fit.commands.clone(), fit.cost.clone(), near.found.clone()))
        u = fit.commands
    return fit, near, [torch.stack([h[i] for h in history]) for i in range(3)]


def _register(s, observed, cells, reach, **kw):
    from neural_jacobian_field_amd.field_volume import register_commands
    count = None if s.count is None else torch.tensor([s.count], dtype=torch.int32, device=s.dev)
    return register_commands(s.tw, _t(s.dev, s.xyz), _t(s.dev, s.labels), observed, cells, reach, joints=s.joints, tree=s.tree,
                             count=count, **kw)


def _same_registration(reg, fit, near, history):
    for f in FIT:
        assert torch.equal(_bytes(getattr(reg.fit, f)), _bytes(getattr(fit, f))), f
    for f in NEAR[:1] + NEAR[3:]:
        assert torch.equal(_bytes(getattr(reg.matches, f)), _bytes(getattr(near, f))), f
    rows = near.index.shape[1] if near.index.numel() else 0
    assert rows and torch.equal(_bytes(reg.matches.distance2), _bytes(near.distance2)) and torch.equal(_bytes(reg.matches.matched), _bytes(near.matched))
    for f, h in zip(HISTORY, history):
        got = getattr(reg, f)
        assert got.dtype == h.dtype and got.shape == h.shape and torch.equal(_bytes(got), _bytes(h)), f


@pytest.mark.parametrize("m", (1, 3))
def test_register_commands_is_the_loop_of_its_public_pieces_on_the_chain(dev, chain, m):
    rng = np.random.default_rng(40 + m)
    planted = np.float32([[0.25, -0.2, 0.0], [-0.4, 0.1, 0.0], [0.1, 0.2, 0.0]])[:m]
    observed = _t(dev, np.stack([p[rng.permutation(272)] for p in chain.targets(planted)]))
    cells, reach = _scene_cells(chain.scene), 4 * chain.scene["step"][0]
    kw = dict(rounds=4, iterations=2, lower=-0.3, upper=torch.tensor([0.3, 0.25, 1.0], device=dev), reg=1e-6, damping=2e-3,
              init=torch.full((m, 3), 0.5, device=dev))
    reg = _register(chain, observed, cells, reach, **kw)
    rounds = kw.pop("rounds")
    _same_registration(reg, *_loop(chain, observed, cells, reach, rounds, kw.pop("iterations"), **kw))
    assert reg.commands_history.shape == (4, m, 3) and reg.cost_history.dtype == torch.float64 and reg.found_history.dtype == torch.int32
    assert torch.equal(reg.commands_history[-1], reg.fit.commands) and torch.equal(reg.found_history[-1], reg.matches.found)
    assert (reg.fit.commands <= torch.tensor([0.3, 0.25, 1.0], device=dev)).all() and (reg.fit.commands >= -0.3).all()


def test_register_commands_is_the_loop_of_its_public_pieces_on_a_face(dev):
    scene = J.face()
    scene["omega"], scene["velocity"] = 0.3 * scene["omega"], 0.05 * scene["velocity"]
    scene["count"] = 3200
    s = Scene(dev, scene, tree=False)
    planted = (0.2 * np.random.default_rng(6).uniform(-1, 1, (2, 10))).astype(np.float32)
    rng = np.random.default_rng(41)
    observed = _t(dev, np.stack([p[rng.permutation(3240)] for p in s.targets(planted)]))
    cells, reach = _scene_cells(scene), 2.5 * max(scene["step"])
    reg = _register(s, observed, cells, reach, rounds=3, iterations=3, observed_count=torch.tensor([3240, 3000], dtype=torch.int32, device=dev))
    _same_registration(reg, *_loop(s, observed, cells, reach, 3, 3, observed_count=torch.tensor([3240, 3000], dtype=torch.int32, device=dev)))
    assert (reg.found_history > 0).all() and not reg.fit.status.any()


# ---- (e) recovery on the device -------------------------------------------------------------------------------------------------------------
def _planted(angles):
    return np.float32([[angles[0] / 0.7, angles[1] / 1.3, 0.0]])


def _observation(s, command, seed, keep=None, nans=0):
    rng = np.random.default_rng(seed)
    posed = s.targets(command)[0]
    if keep is not None:
        posed = posed[keep]
    posed = np.concatenate([posed, np.full((nans, 3), np.nan, np.float32)])
    return posed[rng.permutation(posed.shape[0])]


@pytest.mark.parametrize("angles", [(0.1, 0.1), (0.2, -0.2), (-0.3, 0.3)])
def test_a_planted_command_is_recovered_from_a_shuffled_cloud(dev, chain, angles):
    planted = _planted(angles)
    reg = _register(chain, _t(dev, _observation(chain, planted, 1)), _scene_cells(chain.scene), 4 * chain.scene["step"][0], rounds=12,
                    iterations=3)
    err = np.abs(_np(reg.fit.commands) - planted).max()
    print(f"angles {angles}: |u - planted| {err:.2e}, cost {reg.fit.cost.tolist()}, found {reg.found_history[:, 0].tolist()}")
    assert err <= RECOVERY and not reg.fit.status.any()


@pytest.mark.parametrize("cells_of_reach", (2, 4))
@pytest.mark.parametrize("angle", (0.2, 0.3))
def test_a_partial_padded_observation_recovers_the_command(dev, chain, angle, cells_of_reach):
    planted = _planted((angle, -angle))
    links = np.flatnonzero(chain.labels != chain.parts[0])
    observed = _t(dev, _observation(chain, planted, 2, keep=links, nans=17))
    reg = _register(chain, observed, _scene_cells(chain.scene), cells_of_reach * chain.scene["step"][0], rounds=8, iterations=3)
    err = np.abs(_np(reg.fit.commands) - planted).max()
    print(f"partial, {angle} rad, reach {cells_of_reach} steps: |u - planted| {err:.2e}, found {reg.found_history[:, 0].tolist()}")
    assert err <= RECOVERY and (reg.found_history < 272).all() and int(reg.found_history[-1, 0]) > 0


def test_several_starts_against_one_observation(dev, chain):
    planted = _planted((0.45, 0.6))
    observed = _t(dev, _observation(chain, planted, 3)[None])
    starts = _t(dev, np.float32([[a / 0.7, b / 1.3, 0.0] for a in (-0.6, 0.0, 0.6) for b in (-0.35, 0.0, 0.35)]))
    reg = _register(chain, observed, _scene_cells(chain.scene), 4 * chain.scene["step"][0], init=starts, rounds=12, iterations=3)
    best = int(reg.fit.cost.argmin())
    err = np.abs(_np(reg.fit.commands) - planted).max(axis=1)
    print(f"nine starts: costs {reg.fit.cost.tolist()}, errors {err.tolist()}, best {best}")
    assert reg.fit.cost.shape == (9,) and reg.matches.index.shape == (9, 272) and err[best] <= RECOVERY


# ---- (f) cloud_registration: two calls, and a capture ---------------------------------------------------------------------------------------
def test_cloud_registration_gives_equal_bytes_and_a_capture_replays_them(dev, chain):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud, cloud_registration
    scene = chain.scene
    cloud = FieldPointCloud(grid=FieldGrid(scene["origin"], scene["step"], scene["dims"]), index=_t(dev, scene["index"]),
                            xyz=_t(dev, chain.xyz), density=torch.ones(272, device=dev), color=None, jacobian=None,
                            count=torch.tensor([272], dtype=torch.int32, device=dev))
    labels = _t(dev, chain.labels)
    observed = _t(dev, np.stack([_observation(chain, _planted(a), 4) for a in ((0.2, 0.1), (-0.1, 0.3))]))
    reach = 4 * scene["step"][0]
    kw = dict(joints=chain.joints, tree=chain.tree, rounds=5)
    first, second = (cloud_registration(cloud, labels, chain.tw, observed, reach, **kw) for _ in range(2))
    direct = _register(chain, observed, _scene_cells(scene), reach, rounds=5)                             # (the default cells)

    def same(a, b):
        for f in FIT:
            assert torch.equal(_bytes(getattr(a.fit, f)), _bytes(getattr(b.fit, f))), f
        for f in NEAR:
            assert torch.equal(_bytes(getattr(a.matches, f)), _bytes(getattr(b.matches, f))), f
        for f in HISTORY:
            assert torch.equal(_bytes(getattr(a, f)), _bytes(getattr(b, f))), f

    same(first, second)
    same(first, direct)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        reg = cloud_registration(cloud, labels, chain.tw, observed, reach, **kw)
    for t in [getattr(reg.fit, f) for f in FIT] + [getattr(reg.matches, f) for f in NEAR] + [getattr(reg, f) for f in HISTORY]:
        t.view(torch.uint8).fill_(0x33)
    graph.replay()
    torch.cuda.synchronize()
    same(reg, first)
    err = np.abs(_np(first.fit.commands) - np.concatenate([_planted((0.2, 0.1)), _planted((-0.1, 0.3))])).max()
    print(f"cloud_registration, 5 rounds: |u - planted| {err:.2e}, found {first.found_history.tolist()}")
    assert (first.found_history > 0).all() and not first.fit.status.any()


# ---- (g) end to end: a model's field, its parts, their twists, joints and poses, and the registration to the posed rows ---------------------
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


def test_cloud_registration_end_to_end(model, dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_components, cloud_joints, cloud_pose, cloud_registration,
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
    u = torch.from_numpy((0.05 / max(speed, 1e-6) * np.random.default_rng(10).uniform(-1, 1, (3, 8))).astype(np.float32)).to(dev)
    _, posed = cloud_pose(cloud, labels, tw, u, joints=joints, tree=tree, first_order_elsewhere=False)
    count = int(cloud.count.item())
    observed = posed[:, torch.from_numpy(np.random.default_rng(11).permutation(count)).to(dev)].contiguous()
    reg = cloud_registration(cloud, labels, tw, observed, 2.0 * max(grid.step), joints=joints, tree=tree, rounds=4)
    print(f"{count} rows, {int(tw.count.item())} parts: found {reg.found_history.tolist()}, cost {reg.cost_history.tolist()}")
    assert (reg.matches.found > 0).all() and not reg.fit.status.any()
    assert (reg.cost_history[-1] <= reg.cost_history[0]).all()
    for t in [getattr(reg.fit, f) for f in FIT] + [reg.cost_history, reg.commands_history]:
        assert torch.isfinite(t.double()).all()
