"""Host-side tests of the normals of an observed cloud (field_volume.point_normals / FieldNormals; njf_field_normals; DESIGN.md
section 21): the numpy restatement (tests/field_normals_restatement.py) -- the integer moments do not depend on the order of
the neighbours, the rings 0 .. R hold every neighbour, the quantisation to radius / 2^18 moves a normal by less than 5e-5 --,
the sign rules, ``information()``, every argument check, raised before any device work (there is no GPU here), and the C
ABI's symbol and return codes."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_normals_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 23
# the quantisation step radius / 2^18 against a neighbourhood spread of about radius / 4: 1.5e-5 per offset, less in a
# covariance of tens of them; 5e-5 leaves room for other seeds
QUANTISATION_SIN = 5e-5
TORUS = ((1500, 0.12, 0.0), (1500, 0.12, 0.004), (400, 0.2, 0.0), (3000, 0.08, 0.002))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


# ---- (i) integer moments ---------------------------------------------------------------------------------------------------------------
def test_the_moments_do_not_depend_on_the_order_of_the_neighbours():
    rng = np.random.default_rng(21)
    worst = 0
    for radius in (0.12, 1e-3, 37.5, 1.0):
        pts = (rng.standard_normal((400, 3)) * radius * 0.7).astype(np.float32)
        pts[:5] = pts[5]                                        # coincident points, the query among them
        for q in (pts[5], pts[77], np.float32([radius, 0, 0]), np.float32([0.3 * radius, -0.2 * radius, 0.0])):
            e = S.offsets(q, pts)
            k = S.quantise(e[S.within(e, radius)], radius)
            assert k.shape[0] >= 3
            worst = max(worst, int(np.abs(k).max()))
            first = S.sums(k)
            for _ in range(3):
                again = S.sums(k[rng.permutation(k.shape[0])])
                assert again.dtype == np.int64 and again.tobytes() == first.tobytes()
            assert first[0] == k.shape[0] and first[4] >= 0 and first[7] >= 0 and first[9] >= 0
    # a neighbour on the sphere itself: d2 <= r2 lets |e_c| reach the radius, and rint one step more at the most
    edge = S.offsets(np.float32([0, 0, 0]), np.float32([[0.12, 0, 0], [0, -0.12, 0], [0, 0, np.nextafter(np.float32(0.12), np.float32(1))]]))
    assert S.within(edge, 0.12).tolist() == [True, True, False]
    worst = max(worst, int(np.abs(S.quantise(edge[:2], 0.12)).max()))
    print(f"max |k| {worst} (2^18 = {2 ** 18})")
    assert 2 ** 17 < worst <= 2 ** 18 + 1


# ---- (ii) the rings 0 .. R hold every neighbour ---------------------------------------------------------------------------------------
def _random_case(rng, kind):
    """A lattice, points and queries: kind 0 generic, 1 lattice-aligned on half cells, 2 degenerate dims / one cell."""
    dims = tuple(int(d) for d in rng.integers(1, 9, 3))
    if kind == 2:
        dims = tuple(1 if rng.random() < 0.6 else d for d in dims)
    cell = np.float32(rng.uniform(0.05, 0.5))
    origin = rng.uniform(-1, 1, 3).astype(np.float32)
    extent = np.asarray(dims) * cell
    mo, mq = [(1, 1), (1, 3), (3, 1), (2, 2)][int(rng.integers(0, 4))]
    t, n = int(rng.integers(1, 160)), int(rng.integers(1, 40))

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
    radius = float(cell) * float(rng.choice([0.3, 0.99, 1.0, 2.5, 6.0]))
    return dict(observed=observed, queries=queries, origin=origin, cell=cell, dims=dims, radius=radius,
                observed_count=observed_count, count=count)


def test_the_rings_hold_every_neighbour():
    rng = np.random.default_rng(2021)
    rows = neighbours = mismatches = saved = 0
    reaches = set()
    for case in range(45):
        c = _random_case(rng, case % 3)
        want = S.brute_moments(c["observed"], c["queries"], c["radius"], c["observed_count"], c["count"])
        got, read = S.ring_moments(**c)
        mismatches += int((got[..., 0] != want[..., 0]).sum())
        assert got.tobytes() == want.tobytes()
        searched = np.broadcast_to(S.N.searched_rows(c["queries"], c["count"]), want.shape[:2])
        assert (want[~searched] == 0).all()                    # rows outside the search: zeros
        rows, neighbours = rows + int(searched.sum()), neighbours + int(want[..., 0].sum())
        valid = S.N.valid_points(c["observed"], c["observed_count"]).sum(axis=1)
        saved += int((np.broadcast_to(valid[:, None], read.shape)[searched] - read[searched]).sum())
        reaches.add(S.ring_count(c["cell"], c["radius"]))
    print(f"rings: {rows} searched rows, {neighbours} neighbours, {mismatches} mismatches in S0, {saved} records not read, R in {sorted(reaches)}")
    assert mismatches == 0 and rows > 1500 and neighbours > 3000 and saved > 0 and {1, 2, 3, 7} <= reaches


def test_the_ring_count():
    assert S.ring_count(0.12, 0.12) == 2 and S.ring_count(0.12, 0.11) == 1 and S.ring_count(0.12 / 2.5, 0.12) == 3
    assert S.ring_count(1.0, 0.99) == 1 and S.ring_count(1.0, 0.995) == 2 and S.ring_count(0.25, 15.75) == 64
    for cell, radius in ((0.1, 0.1), (0.3, 0.05), (0.05, 0.3), (1.0, 62.9)):
        r = S.ring_count(cell, radius)
        assert r >= 1 and (r - 1.0 / 128.0) * cell > radius and (r == 1 or not (r - 1 - 1.0 / 128.0) * cell > radius * (1 + 1e-6))


# ---- (iii) the quantisation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,radius,noise", TORUS)
def test_quantised_normals_follow_the_float64_pca(n, radius, noise):
    pts, truth = S.torus(n, seed=21, noise=noise)
    ref = S.normals(pts, pts, radius)
    plain, lam = S.float_pca(pts, pts, radius)
    has = ref["has"][0]
    assert (has == np.isfinite(plain).all(axis=1)).all()
    sin = S.sines(ref["normal64"][0][has], plain[has])
    gap = (ref["lam"][0][has][:, 1] - ref["lam"][0][has][:, 0]) / ref["lam"][0][has][:, 2]
    few = int((ref["neighbours"][0] < 6).sum())
    to_truth = S.sines(ref["normal64"][0][has], truth[has])
    print(f"torus n {n} radius {radius} noise {noise}: worst |sin| quantised against float64 {sin.max():.2e}; smallest gap "
          f"(l1 - l0) / l2 {gap.min():.2e}; {few} rows below 6 neighbours, {int((~has).sum())} without a normal; neighbours "
          f"{ref['neighbours'][0].min()}..{ref['neighbours'][0].max()}; |sin| to the torus' own normal: median "
          f"{np.median(to_truth):.2e}, max {to_truth.max():.2e}")
    assert has.sum() >= 0.99 * n
    assert sin.max() <= QUANTISATION_SIN
    np.testing.assert_allclose(ref["eigenvalues"][0][has], lam[has], rtol=0, atol=2e-5 * radius * radius)


# ---- (iv) sign rules, information(), signatures --------------------------------------------------------------------------------------
def test_the_sign_rules():
    n = np.array([[0.6, -0.8, 0.0], [-0.8, 0.6, 0.0], [0.5, 0.5, -np.sqrt(0.5)], [-0.6, 0.0, -0.8], [2 ** -0.5, -(2 ** -0.5), 0.0],
                  [-(2 ** -0.5), 2 ** -0.5, 0.0]])
    q = np.zeros((1, 6, 3), np.float32)
    out, margin = S.orient(n[None], q)
    assert np.sign(out[0][:, :]).tolist() == [[-1, 1, 0], [1, -1, 0], [-1, -1, 1], [1, 0, 1], [1, -1, 0], [1, -1, 0]]
    assert margin[0][4] == 0.0 and margin[0][0] == pytest.approx(0.2)
    # with a viewpoint: towards it; a non-finite viewpoint counts as none
    out, margin = S.orient(n[None], q, viewpoint=np.float32([[0, 0, -5]]))
    assert (out[0][[2, 3], 2] < 0).all() and margin[0][3] == pytest.approx(0.8)
    away = S.orient(n[None], q, viewpoint=np.float32([[0, 0, 5]]))[0]
    assert (away[0][[2, 3]] == -out[0][[2, 3]]).all()
    free = S.orient(n[None], q, viewpoint=np.float32([[0, np.nan, 5]]))[0]
    assert free.tobytes() == S.orient(n[None], q)[0].tobytes()
    # a plane seen from either side
    rng = np.random.default_rng(5)
    plane = np.concatenate([rng.uniform(-1, 1, (200, 2)), np.zeros((200, 1))], axis=1).astype(np.float32)
    for v, want in (([0, 0, 3], 1.0), ([0, 0, -3], -1.0), (None, 1.0)):
        ref = S.normals(plane, plane[:20], 0.5, viewpoint=None if v is None else np.float32([v]))
        assert ref["has"].all() and np.abs(ref["normal"][0] - np.float32([0, 0, want])).max() <= 1e-6
        assert np.abs(ref["variation"]).max() <= 1e-12 and (ref["neighbours"] >= 3).all()


def test_the_finish_fills_rows_without_a_normal():
    pts = np.float32([[0, 0, 0]] * 4 + [[5, 0, 0], [5.01, 0, 0], [5, 0.01, 0], [9, 9, 9], [np.nan, 0, 0]])
    ref = S.normals(pts, pts, 0.1, count=8)
    assert ref["neighbours"][0].tolist() == [4, 4, 4, 4, 3, 3, 3, 1, 0]
    assert ref["has"][0].tolist() == [False] * 4 + [True] * 3 + [False] * 2          # coincident; a triangle; alone; not searched
    assert np.isnan(ref["normal"][0][~ref["has"][0]]).all() and np.isnan(ref["variation"][0][~ref["has"][0]]).all()
    assert np.abs(np.abs(ref["normal"][0][4:7]) - np.float32([0, 0, 1])).max() <= 1e-6 and (ref["normal"][0][4:7, 2] > 0).all()
    assert not S.normals(pts, pts, 0.1, min_neighbours=4)["has"][0][4:7].any()
    assert S.normals(pts, pts, 0.1, count=5)["neighbours"][0].tolist() == [4, 4, 4, 4, 3, 0, 0, 0, 0]


def _field_normals(normal, variation):
    from neural_jacobian_field_amd.field_volume import FieldNormals
    normal = torch.tensor(normal, dtype=torch.float32)
    return FieldNormals(normal=normal, neighbours=torch.zeros(normal.shape[:-1], dtype=torch.int32),
                        variation=torch.tensor(variation, dtype=torch.float32),
                        moments=torch.zeros(*normal.shape[:-1], 10, dtype=torch.int64), eigenvalues=None)


def test_information_frees_rows_without_a_normal_and_rows_above_the_variation():
    from neural_jacobian_field_amd.field_volume import INFORMATION_FLOOR, plane_information
    nan = float("nan")
    out = _field_normals([[[0, 0, 1], [nan, nan, nan], [0.6, 0.8, 0], [1, 0, 0]]], [[0.0, nan, 0.05, 0.2]])
    info = out.information()
    assert info.shape == (1, 4, 6) and info.dtype == torch.float32
    assert torch.isnan(info[0, 1]).all() and torch.isfinite(info[0, [0, 2, 3]]).all()
    assert torch.equal(info[0, [0, 2, 3]], plane_information(out.normal[0, [0, 2, 3]]))
    f = INFORMATION_FLOOR
    assert info[0, 0].tolist() == [f, 0, 0, f, 0, 1.0]
    capped = out.information(max_variation=0.05)                  # inclusive
    assert torch.isnan(capped[0, [1, 3]]).all() and torch.equal(capped[0, [0, 2]], info[0, [0, 2]])
    assert torch.isnan(out.information(max_variation=0)[0, 1:]).all()
    assert torch.equal(out.information(max_variation=1.0)[0, [0, 2, 3]], info[0, [0, 2, 3]])
    for bad in (-0.1, nan, "0.1", True):
        with pytest.raises(ValueError, match="FieldNormals.information: max_variation must be"):
            out.information(max_variation=bad)


def test_the_signatures():
    from neural_jacobian_field_amd import field_volume as fv
    keywords = dict(observed_count=None, count=None, viewpoint=None, min_neighbours=3, eigenvalues=False)
    params = inspect.signature(fv.point_normals).parameters
    assert list(params) == ["queries", "observed", "cells", "radius"] + list(keywords)
    assert {k: params[k].default for k in keywords} == keywords
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    assert list(fv.FieldNormals.__dataclass_fields__) == ["normal", "neighbours", "variation", "moments", "eigenvalues"]
    params = inspect.signature(fv.FieldNormals.information).parameters
    assert list(params) == ["self", "max_variation"] and params["max_variation"].default is None


def test_point_normals_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, cell_grid, point_normals
    q, obs = torch.zeros(2, 40, 3), torch.zeros(2, 50, 3)
    cells = cell_grid((0, 0, 0), (1, 1, 1), 0.1)
    for bad in (q.double(), q[..., :2], q[0, 0], np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="point_normals: queries must be fp32"):
            point_normals(bad, obs, cells, 0.1)
    for bad in (obs.double(), obs[..., :2], obs[0, 0], None, torch.zeros(2, 0, 3)):
        for queries in (q, None):
            with pytest.raises(ValueError, match="point_normals: observed must be fp32"):
                point_normals(queries, bad, cells, 0.1)
    with pytest.raises(ValueError, match="point_normals: observed and queries hold one set or one per problem"):
        point_normals(q, torch.zeros(3, 50, 3), cells, 0.1)
    for bad in (None, (0, 0, 0)):
        with pytest.raises(ValueError, match="point_normals: cells must be a FieldGrid"):
            point_normals(q, obs, bad, 0.1)
    with pytest.raises(ValueError, match="point_normals: cells must have three equal steps > 0"):
        point_normals(q, obs, FieldGrid((0, 0, 0), (0.1, 0.1, 0.2), (4, 4, 4)), 0.1)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, "1", None, True):
        with pytest.raises(ValueError, match="point_normals: radius must be a finite number > 0"):
            point_normals(q, obs, cells, bad)
    for bad in (63.001 * float(np.float32(0.1)), 100.0, 1e39):
        with pytest.raises(ValueError, match="point_normals: radius may span at most 63 cells"):
            point_normals(q, obs, cells, bad)
    with pytest.raises(ValueError, match="point_normals: observed_count must be int32 \\[2\\]"):
        point_normals(q, obs, cells, 0.1, observed_count=torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="point_normals: count must be one int32"):
        point_normals(q, obs, cells, 0.1, count=3)
    for bad in (torch.zeros(4), torch.zeros(3).double(), torch.zeros(0, 3), torch.zeros(1, 1, 3), [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError, match="point_normals: viewpoint must be fp32"):
            point_normals(q, obs, cells, 0.1, viewpoint=bad)
    with pytest.raises(ValueError, match="point_normals: observed and queries hold one set or one per problem"):
        point_normals(q, obs, cells, 0.1, viewpoint=torch.zeros(3, 3))
    for bad in (2, 0, -1, 3.0, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="point_normals: min_neighbours must be an integer >= 3"):
            point_normals(q, obs, cells, 0.1, min_neighbours=bad)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="point_normals: eigenvalues must be True or False"):
            point_normals(q, obs, cells, 0.1, eigenvalues=bad)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="point_normals: observed must live on the device of queries"):
            point_normals(q.cuda(), obs, cells, 0.1)
    for args, kw in (((q, obs), {}), ((q[0], obs[0]), {}), ((None, obs), {}), ((None, obs[0]), dict(viewpoint=torch.zeros(3))),
                     ((q[0], obs[0]), dict(viewpoint=torch.zeros(4, 3))),
                     ((q, obs), dict(observed_count=torch.ones(2, dtype=torch.int32), count=torch.ones(1, dtype=torch.int32),
                                     viewpoint=torch.zeros(2, 3), min_neighbours=6, eigenvalues=True))):
        with pytest.raises(ValueError, match="point_normals: .*no CPU path"):
            point_normals(*args, cells, 0.3, **kw)


# ---- (v) the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "njf_field_normals" in declared and "njf_field_normals" in hip.EXPORTED_SYMBOLS and hasattr(lib, "njf_field_normals")
    params = re.search(r"njf_field_normals\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_normals.argtypes) == ARGUMENTS
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_NORMALS_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_NORMALS_ALL"] == hip.FIELD_NORMALS_ALL == sum(hip.FIELD_NORMALS_PHASES) == 7
    assert [defines[f"NJF_FIELD_NORMALS_{n.upper()}"] for n in hip.FIELD_NORMALS_PHASE_NAMES] == list(hip.FIELD_NORMALS_PHASES)
    assert defines["NJF_FIELD_NORMALS_WAVE"] == hip.FIELD_NORMALS_WAVE == 8
    assert defines["NJF_FIELD_NORMALS_MOMENTS_PER_ROW"] == hip.FIELD_NORMALS_MOMENTS_PER_ROW == S.MOMENTS == 10
    assert defines["NJF_FIELD_NORMALS_SWEEPS"] == hip.FIELD_NORMALS_SWEEPS
    assert "#define NJF_FIELD_NORMALS_WORKSPACE(Mo, C, T) NJF_FIELD_NEAREST_WORKSPACE(Mo, C, T)" in header
    assert hip.field_normals_workspace(3, 1000, 77) == hip.field_nearest_workspace(3, 1000, 77) == 3 * 1001 + 3 * 1000 + 4 * 3 * 77 + 3


def test_the_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("observed", "observed_count", "num_observed", "points", "queries", "count", "num_queries", "n", "num_problems", "cells",
             "radius", "min_neighbours", "viewpoint", "num_viewpoints", "moments", "normal", "neighbours", "variation", "eigenvalues",
             "workspace", "workspace_words", "phases")
    assert len(names) + 1 == ARGUMENTS
    need = hip.field_normals_workspace(5, 8 * 9 * 10, 5000)

    def call(origin=(0.0, 0.0, 0.0), step=(0.25, 0.25, 0.25), dims=(8, 9, 10), **kw):
        args = {k: P for k in names}
        args.update(num_observed=5, points=5000, num_queries=5, n=300, num_problems=5, radius=0.5, min_neighbours=3, num_viewpoints=5,
                    workspace_words=need, phases=7, cells=hip.make_field_grid(origin, step, dims))
        args.update(kw)
        return lib.njf_field_normals(*[args[k] for k in names], None)

    for key, values in (("num_problems", (0, -1, 65536)), ("num_observed", (0, 2, 6)), ("num_queries", (0, 4, -5)),
                        ("num_viewpoints", (0, 2, 6)), ("phases", (0, -1, 8, 9, 12, 13, 16)), ("min_neighbours", (2, 0, -3)),
                        ("radius", (0.0, -1.0, float("nan"), float("inf"), 1e-60, 15.76, 1e39))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)
    for dims in ((0, 9, 10), (8, -1, 10), (8, 9, 1025)):
        assert call(dims=dims) == E_VALUE
    for step in ((0.25, 0.25, 0.5), (0.0, 0.0, 0.0), (-0.25,) * 3, (float("nan"),) * 3, (float("inf"),) * 3, (1e-45,) * 3):
        assert call(step=step) == E_VALUE, step
    assert call(origin=(0.0, float("nan"), 0.0)) == E_VALUE
    assert call(dims=(1024, 1024, 512), workspace_words=2 ** 62) == E_VALUE               # 5 * 2^29 cells
    assert call(n=-1) == E_SHAPE
    assert call(points=0) == E_SHAPE
    assert call(points=2 ** 26, workspace_words=2 ** 62) == E_SHAPE                       # the int64 second moments
    assert call(points=2 ** 26 - 1, workspace_words=2 ** 62, workspace=None) == E_NULL    # the last permitted T
    assert call(points=2 ** 29, num_observed=1, workspace_words=2 ** 62) == E_SHAPE
    assert call(workspace_words=need - 1) == E_SHAPE
    assert call(workspace_words=0, phases=4, normal=None) == E_NULL                       # the finish alone needs no workspace
    for key in ("observed", "queries", "cells", "moments", "normal", "neighbours", "variation", "workspace"):
        assert call(**{key: None}) == E_NULL, key
    # a viewpoint that is not given has no count to check; the eigenvalues are optional
    assert call(viewpoint=None, num_viewpoints=0, eigenvalues=None, workspace=None) == E_NULL
    # the build needs no query and no output, the moments no observed points and no normal, the finish no workspace
    assert call(phases=1, observed=None) == E_NULL and call(phases=1, workspace=None, queries=None, moments=None) == E_NULL
    assert call(phases=2, moments=None) == E_NULL and call(phases=10, queries=None, observed=None, normal=None) == E_NULL
    assert call(phases=4, workspace=None, observed=None, queries=None) == E_NULL
    assert call(phases=6, observed=None, variation=None) == E_NULL
    assert call(radius=15.75, moments=None) == E_NULL                                     # 63 cells: the last permitted radius
