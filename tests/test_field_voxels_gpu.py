"""GPU tests of the voxel centroids of a cloud (field_volume.voxel_reduce / FieldVoxels; njf_field_voxels)
against the numpy restatement of their semantics (tests/field_voxels_restatement.py).

Every output is held to the restatement EXACTLY -- the integer sums, counts and cell indices as integers, the centroids byte
for byte: they are one float64 expression of those integers --, in both forms of the reduce launch, whatever the order of the
records inside a cell.  The composition tests feed the result to ``nearest_points``, ``point_normals`` and, from a depth image
through ``depth_points``, to ``register_commands``.

End to end (test_a_depth_image_registers_the_chain_raw_and_reduced): a 48 x 64 depth image of the chain posed at hinge angles
(-0.15, 0.25) rad has 792 pixels with a depth, of which max_jump = 0.05 keeps 686, reduced to 138 centroids of 0.06 cells.
register_commands from zero (the 327 model rows on faces turned to the camera, max_distance 0.4, 12 rounds of 3 iterations)
ends |u - planted| = 1.534e-2 from the raw back-projection and 1.376e-2 from the centroids (asserted: at most 3 times the
first).  Normals of the torus reduced to 3,280 centroids of 0.04 cells: rms |sin| to the analytic normal 3.138e-2 against 1.992e-2
for the same call on the 20,000 raw points (asserted: at most twice).

Run with -m gpu."""
import numpy as np
import pytest
import torch

import block_offsets_cases as K
import field_joints_restatement as J
import field_normals_restatement as NS
import field_voxels_restatement as S
from test_field_commands_gpu import Scene
from test_field_nearest_gpu import _register, _scene_cells
from test_field_normals_gpu import _shell

pytestmark = pytest.mark.gpu

OUT = ("points", "weight", "cell", "sums", "count", "outside")
LATTICES = ((33, 31, 1), (32, 32, 1), (41, 25, 1), (1, 1, 1), (3, 5, 7))     # 1,023, 1,024 and 1,025 cells: the scan block +- 1
ROWS = (1, 63, 64, 65, 257, 4097)


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


def _outputs(dev, m, capacity, fill=None):
    out = dict(points=torch.empty(m, capacity, 3, device=dev), weight=torch.empty(m, capacity, dtype=torch.int32, device=dev),
               cell=torch.empty(m, capacity, dtype=torch.int32, device=dev), sums=torch.empty(m, capacity, 3, dtype=torch.int64, device=dev),
               count=torch.empty(m, dtype=torch.int32, device=dev), outside=torch.empty(m, dtype=torch.int32, device=dev))
    if fill is not None:
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
    return out


def _raw(dev, points, cells, phase, capacity, fill=None, out=None, workspace=None, **kw):
    """hip.field_voxels on outputs of the test's own, optionally sentinel-filled; a dict of tensors."""
    from neural_jacobian_field_amd import hip
    m = points.shape[0] if torch.is_tensor(points) else points[0]
    out = _outputs(dev, m, capacity, fill) if out is None else out
    hip.field_voxels(points, cells.c_grid(), out, phase=phase, workspace=workspace, **kw)
    return out


def _same(got, want, what):
    for f in OUT:
        g = _np(got[f]) if isinstance(got, dict) else _np(getattr(got, f))
        assert g.dtype == want[f].dtype and g.shape == want[f].shape, (what, f, g.dtype, g.shape)
        differ = int((g.view(np.uint8) != want[f].view(np.uint8)).sum())
        assert differ == 0, (what, f, differ)


def _check(dev, points, cells, count=None, min_points=1, capacity=None, what=""):
    """The device, in both forms of the reduce launch, against the restatement: equal bytes in all six outputs."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import voxel_reduce
    p3 = points if points.ndim == 3 else points[None]
    want = S.voxels(p3, cells.origin, cells.step[0], cells.dims, count, min_points, capacity)
    got = voxel_reduce(_t(dev, points), cells, count=_t(dev, count), min_points=min_points, capacity=capacity)
    _same(got, want, what)
    wave = _raw(dev, _t(dev, p3), cells, hip.FIELD_VOXELS_ALL | hip.FIELD_VOXELS_WAVE, want["weight"].shape[1], fill=0x5a,
                points_count=_t(dev, count), min_points=min_points)
    _same(wave, want, what + " (wave)")
    return got, want


def _cloud(rng, sets, rows, cells, outside=0.15, dirty=True):
    """Points over the lattice's box and ``outside`` of its extent beyond it; a few non-finite rows."""
    extent = np.asarray(cells.dims) * cells.step[0]
    pts = (np.asarray(cells.origin) + rng.uniform(-outside, 1 + outside, (sets, rows, 3)) * extent).astype(np.float32)
    if dirty and rows >= 8:
        pts[:, 3, 1], pts[:, rows // 2, 0], pts[:, -2] = np.nan, np.inf, -np.inf
    return pts


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", LATTICES)
def test_every_output_equals_the_restatement(dev, dims):
    rng = np.random.default_rng(sum(dims))
    cells = _cells((-0.37, 0.11, 2.5), 0.043, dims)
    kept = []
    for rows in ROWS:
        for sets in (1, 3):
            pts = _cloud(rng, sets, rows, cells)
            count = None if sets == 1 else np.int32([rows, max(rows // 2, 1), max(rows - 3, 0)])
            _, want = _check(dev, pts if sets == 3 else pts[0], cells, count=count, what=f"{dims} T {rows} Mo {sets}")
            kept.append(int(want["count"].max()))
    print(f"{dims}: kept cells per case {kept}")
    assert kept[-1] == 1 if dims == (1, 1, 1) else kept[-1] >= 64
    _check(dev, _cloud(rng, 3, 257, cells), cells, min_points=2, what=f"{dims} min_points 2")


@pytest.mark.parametrize("dims,clouds", K.CELL_CASES)
def test_a_cell_list_past_256_scan_blocks(dev, dims, clouds):
    """The stride-1,024 instance of the one-workgroup scan with two sums per thread, in the list's build and again over the kept
    flags: 287,430 positions (281 scan blocks) of one cloud, 291,870 (286) of three, whose boundaries fall inside a thread's
    run.  Two points each around the centres of the cells at the ends of the first scan blocks, on both sides of block 256, on
    both sides of the seam between two clouds and in the last position (tests/test_block_primitives_cpu.py)."""
    case = K.cell_case(dims, clouds)
    cells = _cells(K.CELL_ORIGIN, K.CELL_SIZE, dims)
    _, want = _check(dev, case["points"], cells, what=f"{dims} x {clouds}")
    blocks = K.workgroups(case["positions"], K.SCAN_BLOCK)
    print(f"scan blocks {blocks}, per {K.per_thread(blocks)}, kept cells {want['count'].tolist()}, outside {want['outside'].tolist()}")
    assert blocks > K.THREADS and want["count"].min() > 2500
    for cloud, _, cell in case["crafted"]:
        row = np.flatnonzero(want["cell"][cloud] == cell)
        assert row.size == 1 and want["weight"][cloud, row[0]] >= K.CRAFTED_PER_CELL
    _check(dev, case["points"], cells, min_points=2, what=f"{dims} x {clouds} min_points 2")


def test_one_crowded_cell_and_a_cloud_that_misses_the_lattice(dev):
    rng = np.random.default_rng(3)
    cells = _cells((0.0, 0.0, 0.0), 0.25, (4, 4, 4))
    crowd = (np.float32([0.5, 0.25, 0.75]) + rng.uniform(0, 0.25, (1, 4097, 3)) * np.float32(0.999)).astype(np.float32)
    got, want = _check(dev, crowd, cells, what="one cell")
    assert want["count"].tolist() == [1] and want["weight"][0, 0] == 4097 and want["cell"][0, 0] == (2 * 4 + 1) * 4 + 3
    assert abs(float(got.points[0, 0, 0]) - 0.625) < 0.01
    miss = np.concatenate([crowd + np.float32(1.0), -crowd, np.full((1, 5, 3), np.nan, np.float32)], axis=1)
    got, want = _check(dev, miss, cells, what="nothing inside")
    assert want["count"].tolist() == [0] and want["outside"].tolist() == [2 * 4097] and torch.isnan(got.points).all()
    _check(dev, np.concatenate([crowd, miss[:, :4097]], axis=0), cells, min_points=4098, what="min_points above every cell")


# ---- 2. the capacity ------------------------------------------------------------------------------------------------------------------------
def test_a_capacity_below_the_kept_count(dev):
    from neural_jacobian_field_amd import hip
    rng = np.random.default_rng(8)
    cells = _cells((-1.0, -1.0, -1.0), 0.125, (16, 16, 16))
    pts = _cloud(rng, 2, 700, cells, outside=0.02)
    count = np.int32([700, 90])
    full = S.voxels(pts, cells.origin, cells.step[0], cells.dims, count)
    kept = full["count"].tolist()
    assert kept[0] > 400 and 40 < kept[1] < 91
    for capacity in (1, kept[1] - 1, kept[0] - 1, kept[0], kept[0] + 5):
        got, want = _check(dev, pts, cells, count=count, capacity=capacity, what=f"capacity {capacity}")
        assert want["count"].tolist() == kept                                       # the TRUE count
        for fill in (0x00, 0xa5):                                                   # every row is written, whatever was there
            out = _raw(dev, _t(dev, pts), cells, hip.FIELD_VOXELS_ALL, capacity, fill=fill, points_count=_t(dev, count))
            _same(out, want, f"capacity {capacity} on {fill:#x}")
    default, _ = _check(dev, pts, cells, count=count, what="capacity None")
    assert default.points.shape == (2, 700, 3)                                      # min(T, C)
    small, _ = _check(dev, pts, _cells((-1.0, -1.0, -1.0), 0.5, (4, 4, 4)), what="capacity None, C < T")
    assert small.points.shape == (2, 64, 3)


# ---- 3. the phases apart ----------------------------------------------------------------------------------------------------------------------
def test_the_phases_one_by_one_and_on_a_workspace_that_nearest_points_built(dev):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import nearest_points
    rng = np.random.default_rng(13)
    cells = _cells((0.2, -0.4, 1.0), 0.07, (9, 11, 6))
    pts = _cloud(rng, 3, 900, cells)
    count = np.int32([900, 333, 0])
    want = S.voxels(pts, cells.origin, cells.step[0], cells.dims, count, 2, 900)
    p, c = _t(dev, pts), _t(dev, count)
    words = hip.field_voxels_workspace(3, cells.num_nodes, 900)
    shape = (3, 900)
    for form in (0, hip.FIELD_VOXELS_WAVE):
        # (a) one phase per call
        workspace = torch.full((words,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        out = _outputs(dev, 3, 900, fill=0x5a)
        _raw(dev, p, cells, hip.FIELD_VOXELS_BUILD, 900, out=out, workspace=workspace, points_count=c, min_points=2)
        _raw(dev, shape, cells, hip.FIELD_VOXELS_REDUCE | form, 900, out=out, workspace=workspace, points_count=c, min_points=2)
        assert _np(out["outside"]).tolist() == want["outside"].tolist()
        assert (_np(out["weight"]).view(np.uint8) == 0x5a).all()                      # the reduce wrote `outside` only
        _raw(dev, shape, cells, hip.FIELD_VOXELS_COMPACT, 900, out=out, workspace=workspace, points_count=c, min_points=2)
        _same(out, want, f"phase by phase, form {form}")
        # (b) REDUCE | COMPACT on the cell list that njf_field_nearest's own build phase wrote
        workspace = torch.full((words,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        hip.field_nearest(p, (1, 0), cells.c_grid(), 0.1, None, 3, observed_count=c, phase=hip.FIELD_NEAREST_BUILD, workspace=workspace)
        out = _raw(dev, shape, cells, hip.FIELD_VOXELS_REDUCE | hip.FIELD_VOXELS_COMPACT | form, 900, fill=0xa5, workspace=workspace,
                   points_count=c, min_points=2)
        _same(out, want, f"on nearest's build, form {form}")
        # (c) after the whole reduction the workspace still answers njf_field_nearest's query phase
        workspace = torch.full((words,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        _same(_raw(dev, p, cells, hip.FIELD_VOXELS_ALL | form, 900, workspace=workspace, points_count=c, min_points=2), want, "whole")
        queries = _t(dev, _cloud(rng, 3, 200, cells, dirty=False))
        near = nearest_points(queries, p, cells, 0.1, observed_count=c)
        again = dict(index=torch.empty(3, 200, dtype=torch.int32, device=dev), distance2=torch.empty(3, 200, device=dev),
                     matched=torch.empty(3, 200, 3, device=dev), found=torch.empty(3, dtype=torch.int32, device=dev))
        hip.field_nearest(shape, queries, cells.c_grid(), 0.1, again, 3, observed_count=c, phase=hip.FIELD_NEAREST_QUERY,
                          workspace=workspace)
        for f, t in again.items():
            assert torch.equal(_bytes(t), _bytes(getattr(near, f))), f
        assert int(near.found.sum()) > 100


def _one_list_case():
    """The smallest case that crosses every edge the three readers share: C = 1,287 cells and L = 2,574 --
    three scan blocks, the last one partial, the boundary between the problems inside the second --, counts (1500, 777), 100
    points of problem 0 in one cell (the wave form strides it twice), NaN rows, points beyond every face; 193 queries (no
    multiple of 64) with the eight corners of the box, rows far outside it and a NaN row; a reach of 2.3 cells (three rings,
    clipped at the faces)."""
    rng = np.random.default_rng(23)
    cells = _cells((0.2, -0.4, 1.0), 0.07, (9, 11, 13))
    origin, cell, dims = np.float32(cells.origin), np.float32(cells.step[0]), np.asarray(cells.dims)
    pts = _cloud(rng, 2, 1500, cells, outside=0.1)
    pts[0, 100:200] = origin + (np.float32([4, 5, 6]) + rng.uniform(0, 1, (100, 3)).astype(np.float32) * np.float32(0.999)) * cell
    pts[1, 40:44, 2], pts[0, 900] = np.nan, np.inf
    queries = _cloud(rng, 2, 193, cells, outside=0.05, dirty=False)
    corners = np.float32([[x, y, z] for x in (0, dims[0]) for y in (0, dims[1]) for z in (0, dims[2])])
    queries[:, :8] = origin + corners * cell
    queries[:, 8:12] = origin + np.float32([[-5, 3, 3], [4, 17, 6], [4, 5, -6], [15, 17, 19]]) * cell      # beyond the reach of the box
    queries[:, 12, 1] = np.nan
    queries[1, 13:] += np.float32(0.01)
    return cells, pts, np.int32([1500, 777]), queries, float(np.float32(2.3) * cell), 6


def test_one_list_feeds_the_three_readers(dev):
    """One build, then njf_field_nearest's query, njf_field_normals' moments and finish and njf_field_voxels' reduce and compact
    on that workspace, each in the lane and in the wave form: every output equals its restatement byte for byte, and the two
    forms equal each other in every byte.  One output cannot: the float64 eigenvalues are a Jacobi iteration's and the
    restatement's are ``eigh``'s, 1e-15 of the largest apart (752 of the 1,125 differ in a last bit); they are held to
    test_field_normals_gpu's bound on the rows with a normal and to the bytes (NaN) on the others.  The fp32 normals and
    variations round both to the same floats here.  The voxels run last: their reduce parks its flags in the cursors, and
    their scan clears them."""
    import field_nearest_restatement as NN
    import test_field_normals_gpu as TN
    from neural_jacobian_field_amd import hip
    cells, pts, count, queries, reach, min_neighbours = _one_list_case()
    origin, cell, dims = cells.origin, cells.step[0], cells.dims
    NN.check_lattice(origin, cell, dims, reach)
    near = NN.rings(pts, queries, origin, cell, dims, reach, observed_count=count)
    moments, _ = NS.ring_moments(pts, queries, origin, cell, dims, reach, observed_count=count)
    normals = NS.finish(moments, queries, reach, min_neighbours)
    vox = S.voxels(pts, origin, cell, dims, count, 2, cells.num_nodes)
    planted = (4 * dims[1] + 5) * dims[2] + 6
    assert vox["weight"][0][vox["cell"][0] == planted].tolist()[0] > 64 and NS.ring_count(cell, reach) == 3
    assert near["rings"].max() >= 3 and ((near["index"] < 0) & (near["rings"] >= 0)).any()          # a searched row without a match
    assert (normals["neighbours"] < min_neighbours).any() and normals["has"].sum() > 300 and vox["outside"].min() > 50
    m, t, n = 2, pts.shape[1], queries.shape[1]
    p, c, q, grid = _t(dev, pts), _t(dev, count), _t(dev, queries), cells.c_grid()
    workspace = torch.full((hip.field_voxels_workspace(m, cells.num_nodes, t),), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    hip.field_nearest(p, (m, n), grid, reach, None, m, observed_count=c, phase=hip.FIELD_NEAREST_BUILD, workspace=workspace)
    got = []
    for wave in (False, True):
        out = dict(index=torch.empty(m, n, dtype=torch.int32, device=dev), distance2=torch.empty(m, n, device=dev),
                   matched=torch.empty(m, n, 3, device=dev), found=torch.empty(m, dtype=torch.int32, device=dev))
        hip.field_nearest((m, t), q, grid, reach, out, m, observed_count=c, workspace=workspace,
                          phase=hip.FIELD_NEAREST_QUERY | (hip.FIELD_NEAREST_WAVE if wave else 0))
        for f in out:
            assert _np(out[f]).tobytes() == near[f].tobytes(), ("nearest", f, wave)
        nrm = TN._raw(dev, (m, t), q, cells, reach, hip.FIELD_NORMALS_MOMENTS | hip.FIELD_NORMALS_FINISH |
                      (hip.FIELD_NORMALS_WAVE if wave else 0), m, fill=0x5a, workspace=workspace, observed_count=c,
                      min_neighbours=min_neighbours)
        assert _np(nrm["moments"]).tobytes() == moments.tobytes() and _np(nrm["neighbours"]).tobytes() == normals["neighbours"].tobytes()
        for f in ("normal", "variation", "eigenvalues"):
            g, w = _np(nrm[f]), normals[f]
            rows = ~normals["has"] if f == "eigenvalues" else np.ones_like(normals["has"])
            print(f"normals {f}, wave {wave}: {int((g != w)[normals['has']].sum())} of {w[normals['has']].size} values differ from eigh's")
            assert g.dtype == w.dtype and g[rows].tobytes() == w[rows].tobytes(), ("normals", f, wave)
        TN._against_eigh(nrm, normals, reach, f"one list, wave {wave}")
        out.update({"normals " + f: v for f, v in nrm.items()})
        red = _raw(dev, (m, t), cells, hip.FIELD_VOXELS_REDUCE | hip.FIELD_VOXELS_COMPACT | (hip.FIELD_VOXELS_WAVE if wave else 0),
                   cells.num_nodes, fill=0xa5, workspace=workspace, points_count=c, min_points=2)
        _same(red, vox, f"one list, wave {wave}")
        out.update({"voxels " + f: v for f, v in red.items()})
        got.append(out)
    for f in got[0]:
        assert torch.equal(_bytes(got[0][f]), _bytes(got[1][f])), (f, "the two forms differ")


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------------------
def test_calls_and_a_captured_replay_give_equal_bytes(dev):
    from neural_jacobian_field_amd.field_volume import voxel_reduce
    rng = np.random.default_rng(17)
    cells = _cells((0.0, 0.0, 0.0), 0.1, (6, 6, 6))
    # 300 points in each of five cells -- where the order of the records is most likely to differ -- and a sprinkling elsewhere
    corners = np.float32([[0.1, 0.1, 0.1], [0.3, 0.2, 0.4], [0.5, 0.5, 0.5], [0.0, 0.4, 0.2], [0.2, 0.0, 0.5]])
    crowd = (corners[:, None] + rng.uniform(0, 0.1, (5, 300, 3)) * np.float32(0.999)).reshape(-1, 3)
    pts = np.concatenate([crowd, _cloud(rng, 1, 500, cells)[0]]).astype(np.float32)
    pts = np.stack([pts[rng.permutation(2000)] for _ in range(2)])
    p = _t(dev, pts)
    kw = dict(count=torch.tensor([2000, 1700], dtype=torch.int32, device=dev), min_points=2)
    want = S.voxels(pts, cells.origin, cells.step[0], cells.dims, [2000, 1700], 2)
    assert (want["weight"] >= 200).sum() >= 9
    first = voxel_reduce(p, cells, **kw)
    _same(first, want, "first")
    for _ in range(6):
        again = voxel_reduce(p, cells, **kw)
        for f in OUT:
            assert torch.equal(_bytes(getattr(again, f)), _bytes(getattr(first, f))), f
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = voxel_reduce(p, cells, **kw)
    for f in OUT:
        getattr(out, f).view(torch.uint8).fill_(0x77)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for f in OUT:
        assert torch.equal(_bytes(getattr(out, f)), _bytes(getattr(first, f))), f


# ---- 5. composition ---------------------------------------------------------------------------------------------------------------------------
def _torus_normal(points, major=0.5):
    """The unit normal of the torus around the z axis at the surface point nearest to each of ``points``, float64."""
    p = np.asarray(points, dtype=np.float64)
    u = np.arctan2(p[:, 1], p[:, 0])
    off = p - np.stack([major * np.cos(u), major * np.sin(u), np.zeros(len(p))], axis=1)
    return off / np.linalg.norm(off, axis=1, keepdims=True)


def test_the_centroids_are_an_observed_cloud_for_the_queries_and_the_normals(dev):
    from neural_jacobian_field_amd.field_volume import cell_grid, nearest_points, point_normals, voxel_reduce
    torus = NS.torus(20000, seed=21, noise=0.004)[0]                                # test_field_normals_gpu's torus, denser
    radius = 0.12
    lower, upper = torus.min(axis=0).tolist(), torus.max(axis=0).tolist()
    vox = voxel_reduce(_t(dev, torus), cell_grid(lower, upper, 0.04))
    kept = int(vox.count[0])
    assert 1500 < kept < 8000 and int(vox.outside[0]) <= 3 and vox.points.shape[1] > kept   # there are fill rows
    search = cell_grid(lower, upper, radius)
    queries = _t(dev, torus[:700])
    with_count = nearest_points(queries, vox.points, search, radius, observed_count=vox.count)
    without = nearest_points(queries, vox.points, search, radius)
    for f in ("index", "distance2", "matched", "found"):
        assert torch.equal(_bytes(getattr(with_count, f)), _bytes(getattr(without, f))), f
    assert int(with_count.found[0]) == 700
    n_count = point_normals(None, vox.points, search, radius, observed_count=vox.count)
    n_plain = point_normals(None, vox.points, search, radius)
    for f in ("normal", "neighbours", "variation", "moments"):
        a, b = getattr(n_count, f), getattr(n_plain, f)
        assert torch.equal(_bytes(a[:, :kept]), _bytes(b[:, :kept])), f              # the rows of the centroids
    assert torch.isnan(n_plain.normal[0, kept:]).all() and not n_plain.neighbours[0, kept:].any()   # the fill rows are no points
    # the normals of the reduced torus against the analytic normal, and the same call on the unreduced torus
    raw = point_normals(None, _t(dev, torus), search, radius)

    def rms_sine(normals, points):
        has = np.isfinite(normals).all(axis=1)
        sin = NS.sines(normals[has], _torus_normal(points[has]))
        return float(np.sqrt((sin ** 2).mean())), float(sin.max()), int(has.sum())

    e_raw, max_raw, n_raw = rms_sine(_np(raw.normal[0]), torus)
    e_vox, max_vox, n_vox = rms_sine(_np(n_count.normal[0, :kept]), _np(vox.points[0, :kept]))
    print(f"torus: {n_raw} of 20000 raw rows with a normal, rms |sin| {e_raw:.3e} (max {max_raw:.3e}); {n_vox} of {kept} centroids, rms "
          f"|sin| {e_vox:.3e} (max {max_vox:.3e})")
    assert n_raw == 20000 and n_vox == kept
    assert e_vox <= 2.0 * e_raw                           # a centroid sits up to half a cell diagonal off the surface


# ---- 6. end to end: a depth image of the posed chain -> points -> centroids -> the command ---------------------------------------------------
HEIGHT, WIDTH, SHELL_MODEL, SHELL_SEEN, ANGLES, MAX_JUMP, CELL, ROUNDS = 48, 64, 2, 12, (-0.15, 0.25), 0.05, 0.06, 12
# The unreduced route counts as converged below CONVERGED: a pixel is about 0.024 wide at the chain's distance (2.0 / (1.3 * 64)),
# the z-buffer takes the nearest of the surface samples in it and the back-projection puts it on the ray of the pixel's centre,
# so a point is displaced by up to half a pixel, 0.012, one-sidedly on a link seen from one side; over a link of 0.4 that is an
# angle of 0.03 and, at 0.7 rad per unit command, a command 0.043 off at the worst.
CONVERGED = 0.05


def _camera():
    ax, ay = 0.1, -0.08
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = rx @ ry, (0.1, 0.05, -0.9)
    k = np.array([[1.3, 0.0, 0.5], [0.0, 2.0, 0.5], [0.0, 0.0, 1.0]])             # a non-square intrinsic
    return k.astype(np.float32)[None], c2w.astype(np.float32)[None]


def _facing_shell(scene, sub, eye):
    """``_shell`` restricted to the faces whose outward normal points to the half-space of ``eye``: a depth camera sees one side
    of a body, and a model row on a face turned away would be matched to points of the side that is seen."""
    o, s = (np.asarray(v, np.float32).astype(np.float64) for v in (J.ORIGIN, J.STEP))
    rows, labels = [], []
    for (x0, nx, y0, ny, z0, nz), part in zip(J.CHAIN_BOXES, scene["parts"]):
        axes = [np.arange((n - 1) * sub + 1) / sub + a for a, n in ((x0, nx), (y0, ny), (z0, nz))]
        g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
        p = o + s * g
        face = np.zeros(len(g), bool)
        for c in range(3):
            for end, sign in ((axes[c][0], -1.0), (axes[c][-1], 1.0)):
                face |= (g[:, c] == end) & (sign * (eye[c] - p[:, c]) > 0)
        rows.append(p[face])
        labels += [part] * int(face.sum())
    return np.concatenate(rows).astype(np.float32), np.array(labels, np.int32)


def _z_buffer(points, k, c2w, height, width):
    """[H,W] fp32: the smallest camera-space z of the points that fall into each pixel, 0 where none does."""
    k, c2w = np.asarray(k, np.float64), np.asarray(c2w, np.float64)
    cam = (np.asarray(points, np.float64) - c2w[:3, 3]) @ c2w[:3, :3]               # R^T (p - t)
    z = cam[:, 2]
    uv = (cam / z[:, None]) @ k.T
    col, row = np.floor(uv[:, 0] * width).astype(np.int64), np.floor(uv[:, 1] * height).astype(np.int64)
    seen = (z > 0) & (col >= 0) & (col < width) & (row >= 0) & (row < height)
    depth = np.full(height * width, np.inf)
    np.minimum.at(depth, row[seen] * width + col[seen], z[seen])
    return np.where(np.isfinite(depth), depth, 0.0).astype(np.float32).reshape(height, width)


def test_a_depth_image_registers_the_chain_raw_and_reduced(dev):
    from neural_jacobian_field_amd.field_volume import cell_grid, depth_points, voxel_reduce
    chain = Scene(dev, J.chain())
    k, c2w = _camera()
    xyz, labels = _facing_shell(chain.scene, SHELL_MODEL, c2w[0, :3, 3].astype(np.float64))
    assert xyz.shape[0] == 327                                                      # of the 878 rows of the whole shell
    s = Scene(dev, chain.scene, given=(chain.tw, chain.joints, chain.tree, xyz, labels))
    fine = Scene(dev, chain.scene, given=(chain.tw, chain.joints, chain.tree, *_shell(chain.scene, SHELL_SEEN)))
    planted = np.float32([[ANGLES[0] / 0.7, ANGLES[1] / 1.3, 0.0]])
    depth = _z_buffer(fine.targets(planted)[0], k[0], c2w[0], HEIGHT, WIDTH)[None]
    seen = int((depth > 0).sum())
    assert 600 < seen < HEIGHT * WIDTH // 2 and (depth[0, 0] == 0).all()             # the chain fills part of the frame
    cloud = depth_points(_t(dev, depth), _t(dev, k), _t(dev, c2w), kind="z", max_jump=MAX_JUMP)
    mask = S.depth_mask(depth, max_jump=MAX_JUMP)
    raw = _np(cloud.points[0])
    assert int(cloud.kept[0]) == int(mask.sum()) and (np.isfinite(raw).all(axis=1) == mask.reshape(-1)).all()
    # every back-projected point lies within a pixel's footprint of the posed surface samples it was rendered from
    ref = S.pinhole_points(depth, k, c2w, "z")[0][mask.reshape(-1)]
    assert np.abs(raw[mask.reshape(-1)] - ref).max() <= 1e-5
    lower, upper = raw[mask.reshape(-1)].min(axis=0), raw[mask.reshape(-1)].max(axis=0)
    vox = voxel_reduce(cloud.points, cell_grid(lower.tolist(), (upper + 1e-3).tolist(), CELL))
    kept = int(vox.count[0])
    assert int(vox.outside[0]) == 0 and int(vox.weight.sum()) == int(cloud.kept[0]) and 50 < kept < int(cloud.kept[0]) // 2
    cells, reach = _scene_cells(chain.scene), 4 * chain.scene["step"][0]
    reg_raw = _register(s, cloud.points[0], cells, reach, rounds=ROUNDS, iterations=3)
    reg_vox = _register(s, vox.points[0], cells, reach, rounds=ROUNDS, iterations=3, observed_count=vox.count)
    d_raw, d_vox = (float(np.abs(_np(r.fit.commands) - planted).max()) for r in (reg_raw, reg_vox))
    print(f"{seen} pixels with a depth, {int(cloud.kept[0])} kept by max_jump {MAX_JUMP}, {kept} centroids of {CELL} cells: |u - planted| "
          f"raw {d_raw:.3e}, reduced {d_vox:.3e}; found {reg_raw.found_history[:, 0].tolist()} and {reg_vox.found_history[:, 0].tolist()}")
    assert not reg_raw.fit.status.any() and not reg_vox.fit.status.any()
    assert d_raw <= CONVERGED                             # the condition: the unreduced route converges
    assert d_vox <= 3.0 * d_raw                           # fewer and displaced points
