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

Run with -m gpu."""
import numpy as np
import pytest
import torch

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


def _select(dev, keep, capacity):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldGrid
    grid = FieldGrid.from_bounds((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), DIMS)
    assert grid.num_nodes == ENTRIES
    values = np.zeros(ENTRIES, np.float32)
    values[keep] = 1.0
    out = None if capacity == 0 else torch.full((capacity,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    hip.field_select(grid.c_grid(), 1, ENTRIES, out, count, values=torch.from_numpy(values).to(dev), threshold=0.5)
    torch.cuda.synchronize()
    want = np.nonzero(values >= 0.5)[0]
    got_count = int(count.item())
    rows = min(got_count, capacity)
    got = np.zeros(0, np.int64) if out is None else out.cpu().numpy()[:rows]
    print("survivors", want.size, "count", got_count, "capacity", capacity)
    assert got_count == want.size
    assert np.array_equal(got, want[:rows])


@pytest.mark.parametrize("name", list(SELECT))
def test_field_select_keeps_exactly_the_pattern(dev, name):
    _select(dev, SELECT[name], ENTRIES)


@pytest.mark.parametrize("capacity", ["0", "1", "survivors - 1"])
def test_field_select_every_third_entry_into_a_short_output(dev, capacity):
    keep = SELECT["every third"]
    _select(dev, keep, len(keep) - 1 if capacity == "survivors - 1" else int(capacity))


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
