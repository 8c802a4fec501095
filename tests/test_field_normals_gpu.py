"""GPU tests of the normals of an observed cloud (field_volume.point_normals / FieldNormals; njf_field_normals; DESIGN.md
section 21) against the numpy restatement of their semantics (tests/field_normals_restatement.py).

The ten integer sums and the neighbour counts are held to the brute-force definition EXACTLY, in both forms of the moments
launch, and the two forms to each other byte for byte in every output.  The normals are held to ``numpy.linalg.eigh`` of the
same integers: |sin| <= 1e-6 (the fp32 rounding of a unit vector, about 1e-7, plus the Jacobi error in double times the
inverse eigenvalue gap, about 1e-12) on the rows whose gap is at least 1e-3 of the largest eigenvalue.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_joints_restatement as J
import field_metric_restatement as M
import field_normals_restatement as S
from test_field_commands_gpu import Scene
from test_field_metric_gpu import _loop, _register, _same_registration

pytestmark = pytest.mark.gpu

OUT = ("normal", "neighbours", "variation", "moments", "eigenvalues")
SIN, GAP, TIE, VARIATION, EIGENVALUES, LEFT_OUT = 1e-6, 1e-3, 1e-4, 1e-6, 1e-9, 0.01


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


def _box_cells(points, cell):
    from neural_jacobian_field_amd.field_volume import cell_grid
    flat = points.reshape(-1, 3)
    flat = flat[np.isfinite(flat).all(axis=1)]
    return cell_grid(flat.min(axis=0).tolist(), flat.max(axis=0).tolist(), cell)


def _outputs(dev, m, n, fill=None):
    out = dict(normal=torch.empty(m, n, 3, device=dev), neighbours=torch.empty(m, n, dtype=torch.int32, device=dev),
               variation=torch.empty(m, n, device=dev), moments=torch.empty(m, n, 10, dtype=torch.int64, device=dev),
               eigenvalues=torch.empty(m, n, 3, dtype=torch.float64, device=dev))
    if fill is not None:
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
    return out


def _raw(dev, observed, queries, cells, radius, phase, m, fill=None, out=None, workspace=None, **kw):
    """hip.field_normals on outputs of the test's own, optionally sentinel-filled; a dict of tensors."""
    from neural_jacobian_field_amd import hip
    out = _outputs(dev, m, queries.shape[1], fill) if out is None else out
    hip.field_normals(observed, queries, cells.c_grid(), radius, out, m, phase=phase, workspace=workspace, **kw)
    return out


def _against_eigh(got, want, radius, what):
    """(b) and (c): the device's finish against ``eigh`` of the same integer moments."""
    has = want["has"]
    normal, variation, eigenvalues = (_np(got[f]) for f in ("normal", "variation", "eigenvalues"))
    assert normal.dtype == np.float32 and variation.dtype == np.float32 and eigenvalues.dtype == np.float64
    assert (np.isfinite(normal).all(axis=-1) == has).all() and (np.isfinite(variation) == has).all(), what
    assert (np.isfinite(eigenvalues).all(axis=-1) == has).all()
    assert np.isnan(normal[~has]).all() and np.isnan(variation[~has]).all()
    lam = want["lam"][has]
    clear = (lam[:, 1] - lam[:, 0]) >= GAP * lam[:, 2]
    searched = int((want["neighbours"] > 0).sum())
    sin = S.sines(normal[has][clear], want["normal64"][has][clear])
    length = np.abs(np.linalg.norm(normal[has].astype(np.float64), axis=-1) - 1.0)
    decided = clear & (want["margin"][has] > TIE)
    same = (normal[has].astype(np.float64) * want["normal64"][has]).sum(axis=-1)[decided] > 0
    dv = np.abs(variation[has].astype(np.float64) - (lam[:, 0] / lam.sum(axis=1)))
    scale = S.SCALE / float(np.float32(radius))
    de = np.abs(eigenvalues[has] - lam / scale ** 2).max(axis=1) / (lam[:, 2] / scale ** 2)
    print(f"{what}: {searched} searched rows, {int(has.sum())} with a normal, {int((~clear).sum())} below the gap; worst |sin| "
          f"{sin.max() if sin.size else 0:.2e}, | |n| - 1 | {length.max() if length.size else 0:.2e}, variation {dv.max() if dv.size else 0:.2e}, "
          f"eigenvalues {de.max() if de.size else 0:.2e} of the largest; signs compared on {int(decided.sum())} rows")
    assert int((~clear).sum()) <= LEFT_OUT * searched
    assert (sin <= SIN).all() and (length <= 1e-6).all() and same.all() and (dv <= VARIATION).all() and (de <= EIGENVALUES).all()
    assert (np.diff(eigenvalues[has], axis=1) >= 0).all() and (eigenvalues[has] >= 0).all()


def _check(dev, observed, queries, cells, radius, observed_count=None, count=None, viewpoint=None, min_neighbours=3, what=""):
    """The device, in both forms of the moments launch, against the restatement: (a) equal integers, equal bytes between the
    forms; (b), (c) the finish."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import point_normals
    want = S.normals(observed, observed if queries is None else queries, radius, observed_count, count, min_neighbours, viewpoint)
    kw = dict(observed_count=_t(dev, observed_count), count=None if count is None else torch.tensor([count], dtype=torch.int32, device=dev),
              viewpoint=_t(dev, viewpoint), min_neighbours=min_neighbours)
    got = point_normals(_t(dev, queries), _t(dev, observed), cells, radius, eigenvalues=True, **kw)
    got = {f: getattr(got, f) for f in OUT}
    o3 = _t(dev, observed if observed.ndim == 3 else observed[None])
    q3 = o3 if queries is None else _t(dev, queries if queries.ndim == 3 else queries[None])
    m = want["moments"].shape[0]
    if kw["viewpoint"] is not None and kw["viewpoint"].dim() == 1:
        kw["viewpoint"] = kw["viewpoint"][None]
    wave = _raw(dev, o3, q3, cells, radius, hip.FIELD_NORMALS_ALL | hip.FIELD_NORMALS_WAVE, m, fill=0x5a, **kw)
    for f in ("moments", "neighbours"):
        lane = _np(got[f])
        assert lane.dtype == want[f].dtype and lane.shape == want[f].shape, f
        differ = int((lane != want[f]).sum())
        assert differ == 0, (what, f, differ)
    for f in OUT:
        assert torch.equal(_bytes(got[f]), _bytes(wave[f])), (what, f, "the two forms differ")
    _against_eigh(got, want, radius, what)
    return got, want


# ---- (a), (b): the torus ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torus():
    return S.torus(1500, seed=21, noise=0.004)[0]


@pytest.mark.parametrize("cell,dims", ((0.12, None), (0.12 / 2.5, None), (2.0, (1, 1, 1))))
def test_the_torus_against_itself(dev, torus, cell, dims):
    cells = _box_cells(torus, cell) if dims is None else _cells((-1.0, -1.0, -1.0), cell, dims)
    got, want = _check(dev, torus, None, cells, 0.12, what=f"torus, cells of {cell:.3f} {cells.dims}")
    assert want["has"].all() and want["neighbours"].min() >= 3 and S.ring_count(cell, 0.12) == {0.12: 2, 2.0: 1}.get(cell, 3)


def _messy(rng, torus, sets, t):
    """``sets`` clouds of ``t`` torus points each, with NaN and inf rows."""
    observed = np.stack([torus[rng.permutation(torus.shape[0])[:t]] for _ in range(sets)])
    observed[rng.random((sets, t)) < 0.04, 1] = np.nan
    observed[rng.random((sets, t)) < 0.03, 2] = np.inf
    return observed


@pytest.mark.parametrize("mo,mq", ((1, 3), (3, 1), (3, 3)))
def test_several_problems_counts_and_queries_off_the_cloud(dev, torus, mo, mq):
    rng = np.random.default_rng(10 * mo + mq)
    observed = _messy(rng, torus, mo, 900)
    queries = np.stack([torus[rng.permutation(1500)[:300]] for _ in range(mq)])
    queries[:, 100:200] += rng.normal(0, 0.03, (mq, 100, 3)).astype(np.float32)        # near the cloud, not of it
    queries[:, 200:230] = rng.uniform(-3, 3, (mq, 30, 3)).astype(np.float32)            # mostly outside the box
    queries[:, ::19, 0] = np.nan
    queries[:, 257:] = np.float32([np.nan, 3e38, -np.inf])                             # garbage behind the count
    cells = _cells((-0.75, -0.75, -0.25), 0.12, (13, 12, 5))
    observed_count = np.int32([900, 450, 0][:mo]) if mo == 3 else np.int32([800])
    viewpoint = np.float32([[0, 0, 0], [np.nan, 0, 0], [9, 9, 9]])
    got, want = _check(dev, observed, queries, cells, 0.12, observed_count=observed_count, count=257, viewpoint=viewpoint,
                       min_neighbours=5, what=f"Mo {mo} Mq {mq}")
    assert (want["neighbours"][:, 257:] == 0).all() and (want["moments"][:, 257:] == 0).all() and want["has"][:, :100].sum() > 50
    if mo == 3:
        assert (want["neighbours"][2] == 0).all() and not want["has"][2].any() and want["neighbours"][1].max() > 5


# ---- (c) fills; nothing is read past the count ------------------------------------------------------------------------------------------
def test_rows_without_a_normal_get_the_fill_and_every_row_is_written(dev):
    from neural_jacobian_field_amd import hip
    rng = np.random.default_rng(3)
    plane = np.concatenate([rng.uniform(0, 1, (400, 2)), np.zeros((400, 1))], axis=1).astype(np.float32)
    pts = np.concatenate([plane, np.float32([[3, 3, 3]] * 5 + [[5, 5, 5], [5.01, 5, 5], [7, 7, 7], [np.nan, 0, 0]])])
    queries = np.concatenate([pts, np.float32([[np.inf, 0, 0]] * 4)])[None]
    count = pts.shape[0]                                                                 # the four rows behind it are not read
    cells = _cells((0, 0, 0), 0.25, (4, 4, 1))
    want = S.normals(pts, queries, 0.1, None, count, 3)
    rows = want["neighbours"][0]
    assert rows[400:405].tolist() == [5] * 5 and rows[405:408].tolist() == [2, 2, 1] and rows[408:].tolist() == [0] * 5
    assert not want["has"][0, 400:].any() and want["has"][0, :400].sum() > 380
    o, q, c = _t(dev, pts[None]), _t(dev, queries), torch.tensor([count], dtype=torch.int32, device=dev)
    outs = []
    for fill in (0x00, 0xa5):
        for wave in (0, hip.FIELD_NORMALS_WAVE):
            out = _raw(dev, o, q, cells, 0.1, hip.FIELD_NORMALS_ALL | wave, 1, fill=fill, count=c)
            assert _np(out["moments"]).tobytes() == want["moments"].tobytes() and _np(out["neighbours"]).tobytes() == want["neighbours"].tobytes()
            _against_eigh(out, want, 0.1, f"fill {fill:#x} wave {wave}")
            outs.append(out)
    for out in outs[1:]:
        for f in OUT:
            assert torch.equal(_bytes(out[f]), _bytes(outs[0][f])), f
    normal = _np(outs[0]["normal"])[0]
    assert np.abs(normal[:400][want["has"][0, :400]] - np.float32([0, 0, 1])).max() <= 1e-6          # the plane, its largest component positive
    # the finish alone does not read the moments of the rows from the count on
    out = _outputs(dev, 1, queries.shape[1], 0xa5)
    out["moments"].copy_(_t(dev, want["moments"]))
    out["moments"][:, count:] = 2 ** 40
    _raw(dev, (1, pts.shape[0]), q, cells, 0.1, hip.FIELD_NORMALS_FINISH, 1, out=out, count=c)
    for f in ("normal", "neighbours", "variation", "eigenvalues"):
        assert torch.equal(_bytes(out[f]), _bytes(outs[0][f])), f


# ---- (d) the phases one by one ---------------------------------------------------------------------------------------------------------------
def test_the_phases_one_by_one(dev, torus):
    from neural_jacobian_field_amd import hip
    rng = np.random.default_rng(4)
    observed = _messy(rng, torus, 1, 1200)
    queries = (torus[:500] + np.float32(0.004))[None]
    cells = _box_cells(torus, 0.1)
    want = S.normals(observed, queries, 0.12, np.int32([1100]), None, 4)
    o, q, oc = _t(dev, observed), _t(dev, queries), torch.tensor([1100], dtype=torch.int32, device=dev)
    full = _raw(dev, o, q, cells, 0.12, hip.FIELD_NORMALS_ALL, 1, observed_count=oc, min_neighbours=4)
    assert _np(full["moments"]).tobytes() == want["moments"].tobytes()
    # the finish fed the restatement's integers
    fed = _outputs(dev, 1, 500, 0x5a)
    fed["moments"].copy_(_t(dev, want["moments"]))
    _raw(dev, (1, 1200), q, cells, 0.12, hip.FIELD_NORMALS_FINISH, 1, out=fed, min_neighbours=4)
    for f in OUT:
        assert torch.equal(_bytes(fed[f]), _bytes(full[f])), f
    # the moments on a cell list that nearest_points' entry built; then build and moments by this entry
    workspace = torch.empty(hip.field_nearest_workspace(1, cells.num_nodes, 1200), dtype=torch.int32, device=dev)
    hip.field_nearest(o, (1, 500), cells.c_grid(), 0.12, None, 1, observed_count=oc, phase=hip.FIELD_NEAREST_BUILD, workspace=workspace)
    for wave in (0, hip.FIELD_NORMALS_WAVE):
        out = _outputs(dev, 1, 500, 0x5a)
        _raw(dev, (1, 1200), q, cells, 0.12, hip.FIELD_NORMALS_MOMENTS | wave, 1, out=out, workspace=workspace)
        assert torch.equal(_bytes(out["moments"]), _bytes(full["moments"])) and (out["neighbours"].view(torch.uint8) == 0x5a).all()
    workspace.fill_(-1)
    _raw(dev, o, (1, 500), cells, 0.12, hip.FIELD_NORMALS_BUILD, 1, out={}, workspace=workspace, observed_count=oc)
    out = _outputs(dev, 1, 500, 0x5a)
    _raw(dev, (1, 1200), q, cells, 0.12, hip.FIELD_NORMALS_MOMENTS | hip.FIELD_NORMALS_FINISH, 1, out=out, workspace=workspace, min_neighbours=4)
    for f in OUT:
        assert torch.equal(_bytes(out[f]), _bytes(full[f])), f


# ---- (e) equal bytes from two calls and from a captured replay -------------------------------------------------------------------------
def test_two_calls_and_a_replay_agree(dev, torus):
    from neural_jacobian_field_amd.field_volume import point_normals
    rng = np.random.default_rng(6)
    o = _t(dev, _messy(rng, torus, 3, 1000))
    q = _t(dev, torus[None, :700] + np.float32(0.002))
    cells = _box_cells(torus, 0.08)
    kw = dict(observed_count=torch.tensor([1000, 500, 40], dtype=torch.int32, device=dev), count=torch.tensor([650], dtype=torch.int32, device=dev),
              viewpoint=torch.tensor([0.0, 0.0, 4.0], device=dev), eigenvalues=True)
    first, second = (point_normals(q, o, cells, 0.12, **kw) for _ in range(2))
    for f in OUT:
        assert torch.equal(_bytes(getattr(first, f)), _bytes(getattr(second, f))), f
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = point_normals(q, o, cells, 0.12, **kw)
    for f in OUT:
        getattr(out, f).view(torch.uint8).fill_(0x77)
    graph.replay()
    torch.cuda.synchronize()
    for f in OUT:
        assert torch.equal(_bytes(getattr(out, f)), _bytes(getattr(first, f))), f
    assert int(torch.isfinite(first.variation).sum()) > 1000 and first.normal.shape == (3, 700, 3)


# ---- (f) the viewpoint --------------------------------------------------------------------------------------------------------------------
def test_normals_face_the_viewpoint(dev, torus):
    from neural_jacobian_field_amd.field_volume import point_normals
    viewpoint = np.float32([[0.0, 0.0, 0.0], [40.0, -30.0, 20.0]])              # in the ring's plane, at its centre; far outside
    got, want = _check(dev, torus, None, _box_cells(torus, 0.12), 0.12, viewpoint=viewpoint, what="two viewpoints")
    normal = _np(got["normal"]).astype(np.float64)
    assert normal.shape == (2, 1500, 3) and np.isfinite(normal).all()
    toward = viewpoint.astype(np.float64)[:, None, :] - torus.astype(np.float64)[None]
    dots = (normal * toward).sum(axis=-1) / np.linalg.norm(toward, axis=-1)
    both = (normal[0] * normal[1]).sum(axis=-1)
    print(f"n . (v - q) / |v - q|: min {dots.min(axis=1)}; the two viewpoints disagree on {int((both < 0).sum())} rows of 1500")
    assert (dots >= -2e-7).all()                                                  # (the sign is set in double; then the fp32 rounding)
    assert (both < 0).sum() > 100 and (both > 0).sum() > 100                      # the two viewpoints see different sides
    single = point_normals(None, _t(dev, torus), _box_cells(torus, 0.12), 0.12, viewpoint=_t(dev, viewpoint[1]))
    assert torch.equal(_bytes(single.normal[0]), _bytes(got["normal"][1]))


# ---- (g) end to end: normals of a noisy observation into point-to-plane registration -------------------------------------------------------
SHELL_SUB, ANGLES, NOISE, RADIUS, REACH, ROUNDS = 2, (0.2, -0.2), 0.002, 0.11, 0.4, 12


def _shell(scene, sub):
    """The chain's three boxes as surfaces: the nodes of a lattice ``sub`` times as fine that lie on a box's faces."""
    o, s = (np.asarray(v, np.float32).astype(np.float64) for v in (J.ORIGIN, J.STEP))
    rows, labels = [], []
    for (x0, nx, y0, ny, z0, nz), part in zip(J.CHAIN_BOXES, scene["parts"]):
        axes = [np.arange((n - 1) * sub + 1) / sub + a for a, n in ((x0, nx), (y0, ny), (z0, nz))]
        g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
        face = np.zeros(len(g), bool)
        for c in range(3):
            face |= (g[:, c] == axes[c][0]) | (g[:, c] == axes[c][-1])
        rows.append(o + s * g[face])
        labels += [part] * int(face.sum())
    return np.concatenate(rows).astype(np.float32), np.array(labels, np.int32)


def test_normals_of_a_noisy_cloud_drive_the_metric_registration(dev):
    from neural_jacobian_field_amd.field_volume import cell_grid, point_normals, ray_information
    chain = Scene(dev, J.chain())
    xyz, labels = _shell(chain.scene, SHELL_SUB)
    s = Scene(dev, chain.scene, given=(chain.tw, chain.joints, chain.tree, xyz, labels))
    planted = np.float32([[ANGLES[0] / 0.7, ANGLES[1] / 1.3, 0.0]])
    rng = np.random.default_rng(21)
    n = xyz.shape[0]
    observed = (s.targets(planted)[0][rng.permutation(n)] + NOISE * rng.standard_normal((n, 3))).astype(np.float32)
    # the restatement's loop on the restatement's normals, and on the identity
    ref = S.normals(observed, observed, RADIUS)
    assert n == 878 and ref["neighbours"].min() >= 6 and ref["has"].all()
    want = M.register(s.twists, xyz, labels, observed, M.plane_information(ref["normal"][0]), REACH, s.parts, s.jd, s.td, rounds=ROUNDS,
                      iterations=3)
    plain = M.register(s.twists, xyz, labels, observed, np.broadcast_to(M.IDENTITY6, (n, 6)), REACH, s.parts, s.jd, s.td, rounds=ROUNDS,
                       iterations=3)
    d_want, d_plain = (float(np.abs(r["fit"]["commands"] - planted).max()) for r in (want, plain))
    # the device
    o = _t(dev, observed)
    cells = cell_grid(observed.min(axis=0).tolist(), observed.max(axis=0).tolist(), RADIUS)
    normals = point_normals(o, o, cells, RADIUS)
    assert np.array_equal(_np(normals.moments), ref["moments"])
    information = normals.information()
    assert information.shape == (1, n, 6) and torch.isfinite(information).all()
    reg = _register(s, o, information, cells, REACH, rounds=ROUNDS, iterations=3)
    _same_registration(reg, *_loop(s, o, information, cells, REACH, ROUNDS, 3))
    identity = _register(s, o, ray_information(normals.normal[0], 1.0), cells, REACH, rounds=ROUNDS, iterations=3)
    d_got, d_identity = (float(np.abs(_np(r.fit.commands) - planted).max()) for r in (reg, identity))
    print(f"{n} rows, noise {NOISE}: |u - planted| with planes {d_got:.3e} (restatement {d_want:.3e}), with the identity {d_identity:.3e} "
          f"(restatement {d_plain:.3e}); cost {reg.fit.cost.tolist()}, found {reg.found_history[:, 0].tolist()}")
    assert not reg.fit.status.any() and int(reg.found_history[-1, 0]) == n
    assert d_got <= max(2.0 * d_want, 1e-6)                                       # the factor 2: the fp32 lattice of the iterate
