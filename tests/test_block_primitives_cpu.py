"""Host-side tests of the cases that put block_offsets_kernel (csrc/njf_kernels.hip) past 256 workgroups:
no GPU, no kernel.  They check the TESTS -- that the sizes, patterns and clouds of tests/block_offsets_cases.py, which the GPU
tests of the selection, the mesh, the band and the cell list run, reach the code they are meant for:

* the regime: more sums than the scan has threads, two or more sums per thread (three at one size), a thread with a short run
  and threads with none at the ragged sizes -- re-derived from the constants of the header and the source;
* the seams: the first sum of a run, a later one, the last run that is not empty and a run that starts at workgroup 256 or
  beyond each carry a count that is not zero in one pattern at the least, at every size;
* the defects: the scan restated with one seam broken (no carry inside a run, no carry from the run scan, ``hi`` not clamped,
  the total taken before the last run) expects other offsets or another total than the scan restated whole in one pattern at
  the least, at every size -- so a kernel with that defect fails a GPU test, checked here without running one.

The scan's restatement itself is held to ``numpy.cumsum``."""
import numpy as np
import pytest

import block_offsets_cases as K
import field_band_restatement as RB
import field_mesh_restatement as RM
import field_nearest_restatement as RN
import field_voxels_restatement as RV


def _assert_past_the_threads(blocks, what):
    r = K.regime(blocks)
    print(what, r)
    assert blocks > K.THREADS and r["per"] >= 2, (what, r)
    assert r["full"] + r["short"] + r["empty"] == K.THREADS and r["short"] <= 1
    assert r["empty"] > 0 and 0 <= blocks - r["full"] * r["per"] < r["per"] and (blocks > r["full"] * r["per"]) == bool(r["short"])
    return r


def _assert_seams_and_defects(cases, what, at_per_one=False, without=()):
    """``cases``: {pattern: per-workgroup sums}, all of one size.  ``without``: the seams and defects a case leaves out on purpose."""
    hit = {}
    seen = {m: [] for m in K.MUTATIONS}
    for name, sums in cases.items():
        sums = [int(v) for v in sums]
        got, total = K.offsets(sums)
        exclusive = np.concatenate([[0], np.cumsum(sums)])
        assert got == exclusive[:-1].tolist() and total == exclusive[-1], (what, name)        # the restatement is a scan
        for seam, carries in K.seams(sums).items():
            hit[seam] = hit.get(seam, False) or carries
        for m in K.MUTATIONS:
            if K.offsets(sums, m) != (got, total):
                seen[m].append(name)
    print(what, "seams", hit, "defects seen by", {m: len(v) for m, v in seen.items()})
    if at_per_one:                     # one sum per run, no run past the threads, nothing to clamp
        without = ("a later sum of a run", "a run that starts at workgroup THREADS or beyond", "no carry inside a run", "hi not clamped")
    for seam, carries in hit.items():
        assert carries != (seam in without), (what, "a count at", seam, carries)
    for m, names in seen.items():
        assert bool(names) != (m in without), (what, "the defect", m, "seen by", names)
    return seen


def test_the_constants_are_the_ones_the_sizes_were_chosen_for():
    from neural_jacobian_field_amd import hip
    assert K.SELECT_BLOCK == K.MESH_BLOCK == K.BAND_BLOCK == hip.FIELD_SELECT_BLOCK == hip.FIELD_MESH_BLOCK == hip.FIELD_BAND_BLOCK
    assert K.SCAN_BLOCK > 0 and K.THREADS > 0 and K.SELECT_BLOCK % K.THREADS == 0
    assert len(K.MUTATIONS) == 4


@pytest.mark.parametrize("blocks", [0, 1, 255, 256, 257, 260, 281, 511, 512, 513, 526, 2048])
def test_the_runs_tile_the_sums(blocks):
    """lo and hi as section 25 states them: contiguous, in order, every sum in one run, none past the end."""
    runs = [K.run(blocks, t) for t in range(K.THREADS)]
    assert runs[0][0] == 0 and runs[-1][1] == blocks and all(0 <= lo <= hi <= blocks for lo, hi in runs)
    assert all(a[1] == b[0] for a, b in zip(runs, runs[1:])) and max(hi - lo for lo, hi in runs) == K.per_thread(blocks)
    sums = (np.arange(blocks) * 7 % 11).tolist()
    exclusive = np.concatenate([[0], np.cumsum(sums)]).astype(np.int64)
    assert K.offsets(sums) == (exclusive[:-1].tolist(), int(exclusive[-1]))


# ---- the selection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", list(K.SELECT_GRIDS))
def test_the_selection_grids(dims):
    entries = dims[0] * dims[1] * dims[2]
    blocks = K.workgroups(entries, K.SELECT_BLOCK)
    r = K.regime(blocks)
    assert (entries, blocks, r["per"], r["full"], r["short"], r["empty"]) == K.SELECT_GRIDS[dims]
    at_per_one = dims == (64, 64, 64)
    if at_per_one:                     # the last size of the other path: one sum per thread, every thread has one
        assert blocks == K.THREADS and r == dict(workgroups=K.THREADS, per=1, full=K.THREADS, short=0, empty=0)
    else:
        _assert_past_the_threads(blocks, f"selection {dims}")
    cases = {}
    for name in K.SELECT_PATTERNS:
        keep = K.select_pattern(name, entries)
        assert keep.size == 0 or (np.diff(keep) > 0).all() and 0 <= keep[0] and keep[-1] < entries
        flags = np.zeros(entries, np.int64)
        flags[keep] = 1
        cases[name] = K.block_sums(flags, K.SELECT_BLOCK)
        assert len(cases[name]) == blocks
    seen = _assert_seams_and_defects(cases, f"selection {dims}", at_per_one)
    if not at_per_one:
        # the pattern written for a seam is among those that see its defect
        assert "the first entry of every workgroup" in seen["no carry inside a run"]
        assert "the entries of workgroups 256 and beyond" in seen["no carry from the run scan"]
        assert "only the last entry" in seen["the total taken before the last run"]
        assert "none" in seen["hi not clamped"]                                             # a total of 0 that is not 0


def test_the_regime_sizes_of_the_selection():
    pers = [K.SELECT_GRIDS[d][2] for d in K.SELECT_GRIDS]
    assert max(pers) >= 3 and pers.count(2) >= 2
    ragged = [d for d, row in K.SELECT_GRIDS.items() if row[4] == 1]
    assert len(ragged) >= 2 and all(K.SELECT_GRIDS[d][5] > 0 for d in ragged)              # a short run, and threads with none
    assert K.SELECT_GRIDS[(65, 64, 64)][3:] == (130, 0, 126)                                # full runs, then none at all


def test_the_list_form_of_the_selection():
    indices, values, count = K.select_list()
    assert indices.size == 268920 == values.size and K.THREADS * K.SELECT_BLOCK < count < indices.size
    blocks = K.workgroups(indices.size, K.SELECT_BLOCK)
    _assert_past_the_threads(blocks, "selection, list form")
    flags = (values >= 0.5).astype(np.int64)
    honoured, ignored = flags.copy(), flags
    honoured[count:] = 0
    sums = K.block_sums(honoured, K.SELECT_BLOCK)
    assert len(sums) == blocks and (sums[K.workgroups(count, K.SELECT_BLOCK):] == 0).all() and sums[K.THREADS:].any()
    assert K.workgroups(count, K.SELECT_BLOCK) < blocks                                     # whole workgroups past the count
    assert K.offsets(K.block_sums(ignored, K.SELECT_BLOCK))[1] > K.offsets(sums)[1]        # a count that is ignored shows
    # the workgroups past the count sum to zero ON PURPOSE: the last run holds nothing, the grids above cover it
    _assert_seams_and_defects({"list": sums}, "selection, list form", without=("the last non-empty run", "the total taken before the last run"))


# ---- the mesh --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes():
    """dims, batch, field -> (per-workgroup vertex sums, per-workgroup triangle sums) of the restatement: computed once."""
    from test_field_mesh_gpu import _analytic, _grid
    out = {}
    for dims, batch, kind in K.MESH_CASES:
        grid = _grid(dims)
        ref = RM.mesh(grid.origin, grid.step, dims, _analytic(grid, kind, batch), 0.0)
        nodes, cells = batch * dims[0] * dims[1] * dims[2], batch * (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
        out[dims, batch, kind] = (np.bincount(ref["vertex_node"] // K.MESH_BLOCK, minlength=K.workgroups(nodes, K.MESH_BLOCK)),
                                  np.bincount(ref["triangle_cell"] // K.MESH_BLOCK, minlength=K.workgroups(cells, K.MESH_BLOCK)))
    return out


def test_the_mesh_cases(meshes):
    expected = {((67, 66, 65), 1): (281, 269), ((53, 52, 53), 2): (286, 270)}
    for size in expected:
        cases = {}
        for (dims, batch, kind), (vertices, triangles) in meshes.items():
            if (dims, batch) != size:
                continue
            assert (len(vertices), len(triangles)) == expected[size]
            _assert_past_the_threads(len(vertices), f"mesh vertices {dims} x {batch} {kind}")
            _assert_past_the_threads(len(triangles), f"mesh triangles {dims} x {batch} {kind}")
            print(kind, "vertex workgroups with a vertex", int((vertices > 0).sum()), "triangle workgroups with one", int((triangles > 0).sum()))
            cases[kind] = (vertices, triangles)
        _assert_seams_and_defects({k: v[0] for k, v in cases.items()}, f"mesh vertices {size}")
        _assert_seams_and_defects({k: v[1] for k, v in cases.items()}, f"mesh triangles {size}")
    vertices = meshes[(67, 66, 65), 1, "random"][0]
    assert (vertices > 0).sum() == 280 and vertices[0] > 0 and vertices[-1] > 0
    vertices = meshes[(67, 66, 65), 1, "sphere"][0]
    filled = np.flatnonzero(vertices)
    assert filled[0] == 56 and len(vertices) - 1 - filled[-1] == 52                          # long runs of zero sums at both ends


# ---- the band --------------------------------------------------------------------------------------------------------------------------
def test_the_band_cases():
    expected = {((65, 65, 73), 1): (308425, 302), ((49, 49, 65), 2): (312130, 305)}
    by_size = {}
    for dims, batch, kind, d in K.BAND_CASES:
        values = K.band_values(dims, batch, kind)
        nodes = batch * dims[0] * dims[1] * dims[2]
        assert (nodes, K.workgroups(nodes, K.BAND_BLOCK)) == expected[dims, batch]
        _assert_past_the_threads(K.workgroups(nodes, K.BAND_BLOCK), f"band {dims} x {batch}")
        active, in_band, index, count = RB.full(values, None, K.BAND_THRESHOLD, dims, K.BAND_FACTOR, d)
        hit = active.any(axis=1)
        assert 0.01 * nodes < count < 0.9 * nodes, "the band must be neither empty nor full"
        sums = K.block_sums(in_band.reshape(-1), K.BAND_BLOCK)
        print(f"band {dims} x {batch} {kind} d {d}: {count} of {nodes} nodes, {int((sums > 0).sum())} of {len(sums)} workgroups")
        if kind == "late":                                   # nothing in front of workgroup 256: the carry arrives late
            assert hit.tolist() == [False] * (batch - 1) + [True]
            assert index[0] >= K.THREADS * K.BAND_BLOCK and not sums[:K.THREADS].any() and sums[-1] > 0
            coarse_x = np.flatnonzero(RB.hits(values, K.BAND_THRESHOLD)[-1]) // ((dims[1] - 1) // K.BAND_FACTOR + 1) // ((dims[2] - 1) // K.BAND_FACTOR + 1)
            assert (coarse_x * K.BAND_FACTOR >= 0.9 * (dims[0] - 1)).all()                    # the hits: the last tenth of x
        by_size.setdefault((dims, batch), {})[kind, d] = sums
    for size, cases in by_size.items():
        _assert_seams_and_defects(cases, f"band {size}")


# ---- the cell list ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,clouds", K.CELL_CASES)
def test_the_cell_list_cases(dims, clouds):
    case = K.cell_case(dims, clouds)
    c, positions = case["cells"], case["positions"]
    assert (positions, K.workgroups(positions, K.SCAN_BLOCK)) == {1: (287430, 281), 3: (291870, 286)}[clouds]
    _assert_past_the_threads(K.workgroups(positions, K.SCAN_BLOCK), f"cell list {dims} x {clouds}")
    RN.check_lattice(K.CELL_ORIGIN, K.CELL_SIZE, dims, K.CELL_REACH)
    assert case["points"].shape == (clouds, K.CELL_ROWS, 3) and case["queries"].shape == (clouds, K.CELL_QUERIES, 3)
    # the crafted points land in the cells they are meant for, by the voxels' rule and by the (clamping) rule of the list's build
    wanted = K.crafted_positions(dims, clouds)
    assert {0, K.SCAN_BLOCK - 1, K.SCAN_BLOCK, 2 * K.SCAN_BLOCK - 1, 2 * K.SCAN_BLOCK, K.THREADS * K.SCAN_BLOCK - 1,
            K.THREADS * K.SCAN_BLOCK, positions - 1} <= set(wanted)
    assert clouds == 1 or {c - 1, c} <= set(wanted)                                           # the last cell of cloud 0, the first of cloud 1
    counts, kept, landed = np.zeros(positions, np.int64), np.zeros(positions, np.int64), {}
    for cloud in range(clouds):
        valid, inside, index, _ = RV.classify(case["points"][cloud], K.CELL_ORIGIN, K.CELL_SIZE, dims)
        assert not valid[[3, K.CELL_ROWS // 2, K.CELL_ROWS - 2]].any() and (valid & ~inside).sum() > 100
        at = RN.cell_of(case["points"][cloud][valid], K.CELL_ORIGIN, K.CELL_SIZE, dims)
        linear = (at[:, 0] * dims[1] + at[:, 1]) * dims[2] + at[:, 2]
        np.add.at(counts, cloud * c + linear, 1)                                              # the build counts every finite point
        assert (linear[inside[valid]] == index[inside]).all()                                  # the two rules agree inside the box
        kept[cloud * c + np.unique(index[inside])] = 1                                        # the flags the voxels' second scan sums
        for which, row, cell in case["crafted"]:
            if which == cloud:
                assert inside[row] and index[row] == cell, (cloud, row, cell, index[row])
                landed[cloud * c + cell] = landed.get(cloud * c + cell, 0) + 1
    assert sorted(landed) == wanted and all(n >= 2 for n in landed.values())
    assert all(counts[p] >= 2 and kept[p] for p in wanted)
    # the queries at the crafted centres find a crafted point of THEIR cell
    near = RN.brute(case["points"], case["queries"], K.CELL_REACH)
    assert near["found"].min() > K.CELL_QUERIES // 2
    rows = {(cloud, row): cell for cloud, row, cell in case["crafted"]}
    first = [0] * clouds
    for position in wanted:
        cloud = position // c
        assert rows[cloud, int(near["index"][cloud, first[cloud]])] == position % c
        first[cloud] += 1
    _assert_seams_and_defects({"counts": K.block_sums(counts, K.SCAN_BLOCK), "kept flags": K.block_sums(kept, K.SCAN_BLOCK)},
                              f"cell list {dims} x {clouds}")
