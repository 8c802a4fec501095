"""GPU tests at the seams of the workgroup primitives (njf_kernels.hip: block_flag_ranks and friends):
survivor patterns that sit on a wave (64), an item (256), a workgroup (1,024) and a chunk (4,096) boundary, through the two
entries that use the ordered compaction in its two roles.

* ``hip.field_select`` on the 13 x 11 x 9 grid (1,287 entries, two workgroups): ``out_indices[:min(count, capacity)]`` and
  ``out_count`` equal ``numpy.nonzero`` of the pattern; rows past the count are not read.
* ``hip.field_twists`` with the pattern as the rows of one part among 4,097 rows (two chunks): ``nodes[0]`` is the pattern's
  size, ``weight`` and ``centroid`` are bit-equal to tests/field_twists_restatement.py.  The coordinates are small integers
  and the weights 1, so every partial sum is exact in double and the correctly rounded sum of the restatement is THE sum in
  any order: a row that is lost, doubled or taken from the wrong place changes the bits, the order of the adds cannot.
  The selection's capacity cases have no counterpart here; the chunk's own seam {4095, 4096} and {0, 4096} stand in.

``block_offsets_kernel`` past its 256 threads.  The scan is one workgroup: thread t owns the run of per = ceil(workgroups / 256)
sums from min(t * per, workgroups) on, thread 0 scans the 256 run totals, every thread rewrites its run.  Up to 256 workgroups
(262,144 entries) per is 1, the loops run once and neither the carry inside a run nor the clamp of a run's end does anything;
every real grid is larger.  ``hip.field_select`` therefore also runs on

    dims           entries   workgroups  per   runs
    64 x 64 x 64   262,144   256         1     the last size of the other path: every thread owns one sum
    65 x 64 x 64   266,240   260         2     threads 0 .. 129 own two, the rest none
    67 x 66 x 65   287,430   281         2     thread 140 owns one, threads 141 .. 255 none
    83 x 81 x 80   537,840   526         3     thread 175 owns one, threads 176 .. 255 none

with eight patterns each -- none, all, only the last entry, the first entry of every workgroup, of the odd workgroups only (the
second sum of every run at per = 2), only the workgroups from 256 on, only the last workgroup, every third entry --, into short
outputs (0, 1, survivors - 1 rows) on the largest, and in the list form: every other node of the largest grid (268,920 entries,
263 workgroups) with a device count of 265,000, so the workgroups 259 .. 262 add zero.  The same regime through the other four
callers: test_field_mesh_gpu.py (both scans of the mesh), test_field_band_gpu.py, test_field_voxels_gpu.py and
test_field_nearest_gpu.py (the cell list's stride-1,024 instance).  The sizes, patterns and clouds live in
tests/block_offsets_cases.py; tests/test_block_primitives_cpu.py re-derives the table from the constants and checks, with the
scan restated and broken in one seam at a time, that each defect changes what these tests expect.  Every case prints its
workgroup count, per and survivor count.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import block_offsets_cases as K
import field_twists_restatement as R

pytestmark = pytest.mark.gpu

DIMS = (13, 11, 9)
ENTRIES = 1287
ROWS = 4097


def _patterns(n):
    return {"none": [], "all": list(range(n)), "wave seam": [63, 64], "item seam": [255, 256], "workgroup seam": [1023, 1024],
            "first and last of 1287": [0, 1286], "every third": list(range(0, n, 3))}


SELECT = _patterns(ENTRIES)
TWISTS = dict(_patterns(ROWS), **{"chunk seam": [4095, 4096], "first and last": [0, ROWS - 1]})


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _select(dev, keep, capacity, dims=DIMS):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldGrid
    grid = FieldGrid.from_bounds((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), dims)
    entries = dims[0] * dims[1] * dims[2]
    assert grid.num_nodes == entries
    values = np.zeros(entries, np.float32)
    values[keep] = 1.0
    out = None if capacity == 0 else torch.full((capacity,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    hip.field_select(grid.c_grid(), 1, entries, out, count, values=torch.from_numpy(values).to(dev), threshold=0.5)
    torch.cuda.synchronize()
    want = np.nonzero(values >= 0.5)[0]
    got_count = int(count.item())
    rows = min(got_count, capacity)
    got = np.zeros(0, np.int64) if out is None else out.cpu().numpy()[:rows]
    blocks = K.workgroups(entries, K.SELECT_BLOCK)
    print("workgroups", blocks, "per", K.per_thread(blocks), "survivors", want.size, "count", got_count, "capacity", capacity)
    assert got_count == want.size
    assert np.array_equal(got, want[:rows])


@pytest.mark.parametrize("name", list(SELECT))
def test_field_select_keeps_exactly_the_pattern(dev, name):
    _select(dev, SELECT[name], ENTRIES)


@pytest.mark.parametrize("capacity", ["0", "1", "survivors - 1"])
def test_field_select_every_third_entry_into_a_short_output(dev, capacity):
    keep = SELECT["every third"]
    _select(dev, keep, len(keep) - 1 if capacity == "survivors - 1" else int(capacity))


# ---- block_offsets_kernel past its 256 threads: runs of two and three sums, the ragged last run, threads with none --------------------
@pytest.mark.parametrize("name", K.SELECT_PATTERNS)
@pytest.mark.parametrize("dims", list(K.SELECT_GRIDS), ids=lambda d: "x".join(map(str, d)))
def test_field_select_past_256_workgroups(dev, dims, name):
    entries = dims[0] * dims[1] * dims[2]
    _select(dev, K.select_pattern(name, entries), entries, dims)


@pytest.mark.parametrize("capacity", ["0", "1", "survivors - 1"])
def test_field_select_past_256_workgroups_into_a_short_output(dev, capacity):
    dims = (83, 81, 80)
    keep = K.select_pattern("every third entry", dims[0] * dims[1] * dims[2])
    _select(dev, keep, keep.size - 1 if capacity == "survivors - 1" else int(capacity), dims)


def test_field_select_on_a_list_whose_count_ends_inside_workgroup_258_of_263(dev):
    """The list form: every other node of the 83 x 81 x 80 grid, a device count of 265,000 -- the workgroups past it add zero."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldGrid
    indices, values, count = K.select_list()
    grid = FieldGrid.from_bounds((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), K.LIST_DIMS)
    capacity = indices.size
    out = torch.full((capacity,), -7, dtype=torch.int32, device=dev)
    out_count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    hip.field_select(grid.c_grid(), 1, capacity, out, out_count, values=torch.from_numpy(values).to(dev), threshold=0.5,
                     indices=torch.from_numpy(indices).to(dev), count=torch.tensor([count], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    want = indices[:count][values[:count] >= 0.5]
    blocks = K.workgroups(capacity, K.SELECT_BLOCK)
    print("workgroups", blocks, "per", K.per_thread(blocks), "of them with entries", K.workgroups(count, K.SELECT_BLOCK), "survivors",
          want.size, "count", int(out_count.item()))
    assert int(out_count.item()) == want.size
    assert np.array_equal(out.cpu().numpy()[:want.size], want)                 # (rows past the count are not read, as in _select)


@pytest.fixture(scope="module")
def rows():
    """Coordinates on a lattice of small integers, a zero Jacobian: computed once, shared, never changed."""
    i = np.arange(ROWS)
    xyz = np.stack([i % 64, (i // 64) % 8, i // 512], axis=1).astype(np.float32)
    return xyz, np.zeros((ROWS, 1, 3), np.float32)


@pytest.mark.parametrize("name", list(TWISTS))
def test_field_twists_sums_exactly_the_pattern(dev, rows, name):
    from neural_jacobian_field_amd import hip
    xyz, jac = rows
    labels = np.zeros(ROWS, np.int32)
    labels[TWISTS[name]] = 1
    parts = np.array([1], np.int32)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    out = dict(labels=torch.empty(1, **i32), count=torch.empty(1, **i32), nodes=torch.empty(1, **i32), status=torch.empty(1, **i32),
               weight=torch.empty(1, **f64), centroid=torch.empty(1, 3, **f64), omega=torch.empty(1, 1, 3, **f64),
               velocity=torch.empty(1, 1, 3, **f64), energy=torch.empty(1, 1, **f64), residual=torch.empty(1, 1, **f64),
               q=torch.empty(1, 6, **f64), p=torch.empty(1, 1, 3, **f64), l=torch.empty(1, 1, 3, **f64),
               row_residual=torch.empty(ROWS, dtype=torch.float32, device=dev))
    hip.field_twists(torch.from_numpy(xyz).to(dev), torch.from_numpy(jac).to(dev), torch.from_numpy(labels).to(dev),
                     torch.from_numpy(parts).to(dev), out)
    torch.cuda.synchronize()
    ref = R.fit(xyz, jac, labels, parts)
    nodes, weight, centroid = out["nodes"].cpu().numpy(), out["weight"].cpu().numpy(), out["centroid"].cpu().numpy()
    print("rows of the part", len(TWISTS[name]), "nodes", nodes, "weight", weight, "centroid", centroid, ref["centroid"])
    assert nodes[0] == len(TWISTS[name]) == ref["nodes"][0]
    assert weight.tobytes() == ref["weight"].tobytes()
    assert centroid.tobytes() == ref["centroid"].astype(np.float64).tobytes()
