"""GPU tests of the connected-component labelling (field_volume.label_components / cloud_components, the
``min_component_nodes`` / ``largest_only`` keywords of extract_field / extract_mesh; njf_field_components).

Everything is integer: every comparison is exact equality of ``labels``, ``sizes`` and ``count`` with the numpy restatement of
the semantics (tests/field_components_restatement.py), and ``status == 0``.  The filtered extractions are compared bit for bit
with the rows / the mesh that the restated components select from the unfiltered ones.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_components_restatement as R

pytestmark = pytest.mark.gpu

IMG = 64
SMALL = (5, 6, 7)        # 210 nodes: less than one workgroup
CRAFTED = (9, 11, 13)    # 1,287 nodes per element, B = 2: the batch boundary and workgroup boundaries fall mid-block
RANDOM = (17, 19, 23)    # 7,429 nodes per element, B = 2: 15 workgroups


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


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


def _grid(dims):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), dims)


def _node(dims, ix, iy, iz):
    return (ix * dims[1] + iy) * dims[2] + iz


def _label(dev, dims, inside, connectivity, keys=None, values=None, threshold=0.5, valid=None):
    """label_components on an occupancy [B, N] (or on explicit values) -> numpy (labels, sizes, count), status asserted 0."""
    from neural_jacobian_field_amd.field_volume import label_components
    if values is None:
        values = inside.astype(np.float32)
    comp = label_components(_grid(dims), torch.from_numpy(values).to(dev), threshold, connectivity=connectivity,
                            keys=None if keys is None else torch.from_numpy(keys.astype(np.int32)).to(dev),
                            valid=None if valid is None else torch.from_numpy(valid).to(dev))
    assert comp.labels.dtype == comp.sizes.dtype == comp.count.dtype == comp.status.dtype == torch.int32
    assert tuple(comp.labels.shape) == tuple(comp.sizes.shape) == tuple(values.shape) and comp.count.shape == comp.status.shape == (1,)
    assert int(comp.status.item()) == 0
    return comp.labels.cpu().numpy(), comp.sizes.cpu().numpy(), int(comp.count.item())


def _assert_equals_restatement(dev, dims, inside, connectivity, keys=None, **kw):
    got = _label(dev, dims, inside, connectivity, keys, **kw)
    ref = R.label(inside, dims, connectivity, keys)
    assert np.array_equal(got[0], ref[0]), ("labels", connectivity)
    assert np.array_equal(got[1], ref[1]), ("sizes", connectivity)
    assert got[2] == ref[2], ("count", connectivity, got[2], ref[2])
    return ref


# ---- 1. crafted cases -----------------------------------------------------------------------------------------------------------
def _empty(dims=CRAFTED, batch=2):
    return np.zeros((batch, dims[0] * dims[1] * dims[2]), dtype=bool)


def test_the_batch_boundary_and_the_grid_faces_do_not_connect(dev):
    dims = CRAFTED
    nodes = dims[0] * dims[1] * dims[2]
    inside = _empty()
    inside[0, nodes - 1] = inside[1, 0] = True                       # the last node of element 0, the first of element 1
    a, b = _node(dims, 3, 4, dims[2] - 1), _node(dims, 3, 5, 0)      # linear neighbours n, n + 1 across a z face
    assert b == a + 1
    inside[0, a] = inside[0, b] = True
    c, d = _node(dims, 2, dims[1] - 1, dims[2] - 1), _node(dims, 3, 0, 0)     # and across a y face
    assert d == c + 1
    inside[1, c] = inside[1, d] = True
    for connectivity in R.CONNECTIVITIES:
        labels, sizes, count = _assert_equals_restatement(dev, dims, inside, connectivity)
        assert count == 6 and (sizes[inside] == 1).all()
        assert labels[0, nodes - 1] == nodes - 1 and labels[1, 0] == nodes


def test_diagonals_join_at_14_only_and_anti_diagonals_never(dev):
    dims = CRAFTED
    inside = _empty()
    p, q = _node(dims, 2, 3, 4), _node(dims, 3, 4, 4)                 # offset (1, 1, 0)
    r, s = _node(dims, 6, 5, 7), _node(dims, 7, 4, 7)                 # offset (1, -1, 0)
    inside[0, [p, q, r, s]] = True
    u, v = _node(dims, 1, 1, 1), _node(dims, 2, 2, 2)                 # offset (1, 1, 1), in element 1
    w, x = _node(dims, 5, 5, 5), _node(dims, 5, 6, 4)                 # offset (0, 1, -1)
    inside[1, [u, v, w, x]] = True
    labels, _, count = _assert_equals_restatement(dev, dims, inside, 6)
    assert count == 8
    labels, sizes, count = _assert_equals_restatement(dev, dims, inside, 14)
    nodes = inside.shape[1]
    assert count == 6 and labels[0, q] == p and labels[0, s] == s and labels[0, r] == r
    assert labels[1, v] == nodes + u and labels[1, w] == nodes + w and labels[1, x] == nodes + x and sizes[0, p] == 2


def test_all_inside_all_outside_and_special_values(dev):
    dims = CRAFTED
    nodes = dims[0] * dims[1] * dims[2]
    for connectivity in R.CONNECTIVITIES:
        labels, sizes, count = _assert_equals_restatement(dev, dims, ~_empty(), connectivity)
        assert count == 2 and (labels[0] == 0).all() and (labels[1] == nodes).all() and (sizes == nodes).all()
        labels, sizes, count = _assert_equals_restatement(dev, dims, _empty(), connectivity)
        assert count == 0 and (labels == -1).all() and (sizes == 0).all()
    # NaN and -inf are outside, a value equal to the threshold is inside (threshold 0.25, exactly representable)
    values = np.full((2, nodes), 0.25, dtype=np.float32)
    values[0, 100:140] = np.nan
    values[0, 300:320] = -np.inf
    values[1, ::3] = np.float32(0.25) - np.spacing(np.float32(0.25))
    values[1, 5::7] = np.inf
    inside = values >= np.float32(0.25)
    assert not inside[0, 100:140].any() and not inside[0, 300:320].any() and inside[0, 0] and not inside[1, 0] and inside[1, 5]
    for connectivity in R.CONNECTIVITIES:
        _assert_equals_restatement(dev, dims, inside, connectivity, values=values, threshold=0.25)


def test_a_valid_mask_cuts_a_bar_in_two(dev):
    dims = CRAFTED
    values = np.zeros((2, dims[0] * dims[1] * dims[2]), dtype=np.float32)
    bar = [_node(dims, ix, 5, 6) for ix in range(dims[0])]            # along x: consecutive nodes lie 143 entries apart
    values[0, bar] = values[1, bar] = 1.0
    valid = np.ones(values.shape, dtype=bool)
    valid[0, bar[4]] = False
    inside = (values >= 0.5) & valid
    for connectivity in R.CONNECTIVITIES:
        labels, sizes, count = _assert_equals_restatement(dev, dims, inside, connectivity, values=values, valid=valid)
        assert count == 3 and sizes[0, bar[0]] == 4 and sizes[0, bar[5]] == 4 and sizes[1, bar[0]] == 9 and labels[0, bar[4]] == -1
    as_u8 = _label(dev, dims, inside, 6, values=values, valid=valid.astype(np.uint8))
    assert np.array_equal(as_u8[0], R.label(inside, dims, 6)[0])


def test_keys_split_and_constant_keys_change_nothing(dev):
    dims = CRAFTED
    inside = ~_empty()
    ix, iy, iz = np.indices(dims)
    checker = np.broadcast_to(((ix + iy + iz) % 2).reshape(1, -1), inside.shape)
    labels, sizes, count = _assert_equals_restatement(dev, dims, inside, 6, keys=checker)
    assert count == inside.size and (sizes == 1).all() and np.array_equal(labels.reshape(-1), np.arange(inside.size))
    rng = np.random.default_rng(5)
    inside = rng.random(inside.shape) < 0.5
    for connectivity in R.CONNECTIVITIES:
        plain = _assert_equals_restatement(dev, dims, inside, connectivity)
        const = _assert_equals_restatement(dev, dims, inside, connectivity, keys=np.full(inside.shape, 7))
        assert np.array_equal(plain[0], const[0]) and np.array_equal(plain[1], const[1]) and plain[2] == const[2]
        _assert_equals_restatement(dev, dims, inside, connectivity, keys=np.broadcast_to(checker, inside.shape))


def test_a_grid_smaller_than_one_workgroup(dev):
    rng = np.random.default_rng(11)
    for batch in (1, 3):
        inside = rng.random((batch, SMALL[0] * SMALL[1] * SMALL[2])) < 0.4
        for connectivity in R.CONNECTIVITIES:
            _assert_equals_restatement(dev, SMALL, inside, connectivity)


# ---- 2. a serpentine path: long find chains across workgroups ----------------------------------------------------------------------
def _serpentine(dims):
    """One-node-wide path through every second row of every second plane of the grid, in visiting order."""
    nx, ny, nz = dims
    path, forward = [], True
    planes = list(range(0, nx, 2))
    for pi, ix in enumerate(planes):
        rows = list(range(0, ny, 2))
        if pi % 2:
            rows.reverse()
        for ri, iy in enumerate(rows):
            zs = range(nz) if forward else range(nz - 1, -1, -1)
            path += [(ix, iy, iz) for iz in zs]
            end = path[-1][2]
            forward = not forward
            if ri + 1 < len(rows):
                path.append((ix, (iy + rows[ri + 1]) // 2, end))      # the connector in the row between
        if pi + 1 < len(planes):
            path.append((ix + 1, path[-1][1], path[-1][2]))           # the connector in the plane between
    return path


@pytest.mark.parametrize("dims", [(12, 12, 12), (20, 20, 20)])
def test_a_serpentine_path_is_one_component(dev, dims):
    path = _serpentine(dims)
    assert len(set(path)) == len(path) > 400
    inside = np.zeros((1, dims[0] * dims[1] * dims[2]), dtype=bool)
    inside[0, [_node(dims, *p) for p in path]] = True
    labels, sizes, count = _assert_equals_restatement(dev, dims, inside, 6)
    assert count == 1 and (sizes[inside] == len(path)).all() and (labels[inside] == 0).all()
    _assert_equals_restatement(dev, dims, inside, 14)
    cut = inside.copy()
    cut[0, _node(dims, *path[len(path) // 2])] = False                # one node removed: two pieces
    assert _assert_equals_restatement(dev, dims, cut, 6)[2] == 2
    flipped = np.stack([inside[0], inside[0][::-1]])                  # and the path run from the far end, as a second element
    _assert_equals_restatement(dev, dims, flipped, 6)


# ---- 3. random occupancy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("occupancy", [0.25, 0.5])
@pytest.mark.parametrize("keyed", [False, True])
def test_random_occupancy_equals_the_restatement(dev, connectivity, occupancy, keyed):
    rng = np.random.default_rng(int(occupancy * 100) + connectivity)
    shape = (2, RANDOM[0] * RANDOM[1] * RANDOM[2])
    inside = rng.random(shape) < occupancy
    keys = rng.integers(0, 3, size=shape) if keyed else None
    labels, sizes, count = _assert_equals_restatement(dev, RANDOM, inside, connectivity, keys)
    assert count > 1 and sizes.max() > 1


@pytest.mark.parametrize("connectivity,occupancy", [(6, 0.32), (14, 0.19), (6, 0.6), (14, 0.6)])
def test_bodies_that_wind_through_many_workgroups(dev, connectivity, occupancy):
    """40^3 = 63 workgroups.  Near the percolation threshold of the adjacency (about 0.31 for the 6 axis neighbours, about 0.18
    for the 14) the largest components are tortuous and cross workgroup boundaries again and again: the unions of launch 2
    contend for few roots and retry.  Well above it one body fills the grid."""
    dims = (40, 40, 40)
    inside = np.random.default_rng(connectivity + int(100 * occupancy)).random((1, 64000)) < occupancy
    labels, sizes, count = _assert_equals_restatement(dev, dims, inside, connectivity)
    assert sizes.max() > (1000 if occupancy < 0.5 else 30000) and count > 1
    if occupancy > 0.5:
        assert _assert_equals_restatement(dev, dims, np.ones((1, 64000), dtype=bool), connectivity)[2] == 1


def test_the_list_form_drops_entries_outside_the_grid_and_past_the_count(dev):
    """njf_field_components on a list: entries outside [0, B*N) name no node and rows past the device count are never read."""
    from neural_jacobian_field_amd import hip
    dims, batch = CRAFTED, 2
    grid = _grid(dims)
    total = batch * grid.num_nodes
    inside = np.random.default_rng(3).random((batch, grid.num_nodes)) < 0.4
    nodes = np.flatnonzero(inside.reshape(-1)).astype(np.int32)
    entries = np.concatenate([[-7, -1], nodes, [total, total + 5, 2 ** 31 - 1]]).astype(np.int32)     # ascending
    padded = np.concatenate([entries, np.full(40, 3, dtype=np.int32)])                              # rows past the count
    keys = np.random.default_rng(4).integers(0, 2, size=padded.size).astype(np.int32)
    dense_keys = np.zeros(total, dtype=np.int32)
    dense_keys[nodes] = keys[2:2 + nodes.size]
    i32 = dict(dtype=torch.int32, device=dev)
    for connectivity in R.CONNECTIVITIES:
        for use_keys in (False, True):
            labels, sizes = torch.empty(total, **i32), torch.empty(total, **i32)
            count, status = torch.empty(1, **i32), torch.empty(1, **i32)
            hip.field_components(grid.c_grid(), batch, connectivity, labels, sizes, count, status,
                                 indices=torch.from_numpy(padded).to(dev), list_count=torch.tensor([entries.size], **i32),
                                 capacity=padded.size, keys=torch.from_numpy(keys).to(dev) if use_keys else None)
            ref = R.label(inside, dims, connectivity, dense_keys.reshape(batch, -1) if use_keys else None)
            assert int(status.item()) == 0 and int(count.item()) == ref[2]
            assert np.array_equal(labels.cpu().numpy(), ref[0].reshape(-1)) and np.array_equal(sizes.cpu().numpy(), ref[1].reshape(-1))


def test_the_frustum_predicate_is_the_selections(dev):
    """``pixel_encoding``: inside needs the node in the context view -- the very predicate of field_select."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import _cameras
    from neural_jacobian_field_amd.field_volume import label_components
    grid, batch = _grid(CRAFTED), 2
    enc = _encoding(batch, dev)
    total = batch * grid.num_nodes
    idx, n = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    hip.field_select(grid.c_grid(), batch, total, idx, n, cams=_cameras(enc, False, action_dim=None))
    seen = np.zeros(total, dtype=bool)
    seen[idx[:int(n.item())].cpu().numpy()] = True
    seen = seen.reshape(batch, -1)
    assert seen.any() and not seen.all()
    values = np.random.default_rng(2).random(seen.shape).astype(np.float32)
    for connectivity in R.CONNECTIVITIES:
        comp = label_components(grid, torch.from_numpy(values).to(dev), 0.3, pixel_encoding=enc, connectivity=connectivity)
        ref = R.label((values >= np.float32(0.3)) & seen, CRAFTED, connectivity)
        assert int(comp.status.item()) == 0 and int(comp.count.item()) == ref[2]
        assert np.array_equal(comp.labels.cpu().numpy(), ref[0]) and np.array_equal(comp.sizes.cpu().numpy(), ref[1])


# ---- 4. keep ----------------------------------------------------------------------------------------------------------------------
def test_keep_equals_the_restatement_including_a_size_tie(dev):
    from neural_jacobian_field_amd.field_volume import label_components
    dims = CRAFTED
    inside = np.random.default_rng(8).random((2, dims[0] * dims[1] * dims[2])) < 0.2
    inside[1] = False
    for base in ((1, 1, 1), (5, 6, 7)):                               # element 1: two bars of five nodes, nothing larger
        inside[1, [_node(dims, base[0], base[1], base[2] + i) for i in range(5)]] = True
    inside[1, _node(dims, 8, 10, 12)] = True
    comp = label_components(_grid(dims), torch.from_numpy(inside.astype(np.float32)).to(dev), 0.5)
    labels, sizes, _ = R.label(inside, dims, 6)
    assert sizes[1].max() == 5 and len(set(labels[1][sizes[1] == 5])) == 2
    for min_nodes, largest_only in ((1, False), (2, False), (5, False), (6, False), (1, True), (3, True), (6, True)):
        got = comp.keep(min_nodes, largest_only)
        assert got.dtype == torch.bool and got.device == comp.labels.device
        assert np.array_equal(got.cpu().numpy(), R.keep(labels, sizes, min_nodes, largest_only)), (min_nodes, largest_only)
    tie = comp.keep(largest_only=True)[1].cpu().numpy()
    assert tie.sum() == 5 and tie[_node(dims, 1, 1, 1)]               # the tie goes to the smallest label


# ---- 5. extractions -----------------------------------------------------------------------------------------------------------------
def _encoding(batch, dev, seed=1):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    c2w = synthetic.general_pose(7, batch, scale=0.04)
    c2w[0] = torch.eye(4)
    k = synthetic.synthetic_cameras(batch)["ctxt_k_norm"]
    return PixelEncoding(features=synthetic.synthetic_features(batch, IMG, IMG, seed=seed).to(dev), extrinsics=c2w.to(dev),
                         intrinsics=k.to(dev), action=synthetic.synthetic_action(batch, 8).to(dev))


CLOUD_FIELDS = ("index", "xyz", "density", "color", "jacobian")
MESH_FIELDS = ("vertex_node", "vertex_edge", "triangles", "triangle_cell", "vertex_t", "vertices")


def _dense_density(model, enc, grid):
    b = enc.extrinsics.shape[0]
    xyz = grid.points(device=enc.extrinsics.device)
    head, _ = model.compute_density(xyz[None].expand(b, -1, 3).contiguous(), enc)
    return head.density.reshape(b, grid.num_nodes).clone()


def _thresholds(model, enc, grid):
    """Candidate thresholds: quantiles of the dense density."""
    d = _dense_density(model, enc, grid).double().cpu().reshape(-1)
    return [float(torch.quantile(d, q)) for q in (0.6, 0.75, 0.45, 0.85, 0.3, 0.93)]


def _restated(cloud, batch, connectivity):
    """The restatement on the node set of an exact cloud: dense (labels, sizes) [B, N] and the cloud's rows as int64."""
    dims, nodes = cloud.grid.dims, cloud.grid.num_nodes
    index = cloud.index.cpu().numpy().astype(np.int64)
    inside = np.zeros(batch * nodes, dtype=bool)
    inside[index] = True
    labels, sizes, _ = R.label(inside.reshape(batch, nodes), dims, connectivity)
    return labels, sizes, index


def _fragmented(extract, thresholds, batch, connectivity=6):
    """An unfiltered cloud whose restated components have at least two distinct sizes, at the first threshold of the list
    that gives one, and K between the sizes: at least one component is dropped and at least one kept."""
    for thr in thresholds:
        cloud = extract(thr)
        if cloud.index.shape[0] < 20:
            continue
        labels, sizes, index = _restated(cloud, batch, connectivity)
        distinct = sorted(set(sizes.reshape(-1)[index].tolist()))
        if len(distinct) >= 2:
            k = distinct[len(distinct) // 2]
            rows = sizes.reshape(-1)[index]
            assert (rows < k).any() and (rows >= k).any()             # the precondition: the filter is not vacuous
            return thr, cloud, labels, sizes, index, k
    raise AssertionError("no threshold of the list fragments the field")


def _rows_equal(a, rows_a, b, rows_b, fields):
    return all(torch.equal(getattr(a, f)[rows_a], getattr(b, f)[rows_b]) for f in fields)


@pytest.mark.parametrize("case", ["single", "cull", "fused"])
def test_extract_field_drops_small_components(model, dev, case):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import cloud_components, extract_field
    grid = _grid((17, 13, 11))
    kw = dict(single={}, cull=dict(cull=0.0), fused=dict(views_per_scene=2))[case]
    enc = _encoding(2, dev)
    batch = 1 if case == "fused" else 2
    model.set_precision("f32")
    try:
        thresholds = _thresholds(model, enc, grid)
        for connectivity in R.CONNECTIVITIES:
            thr, full, labels, sizes, index, k = _fragmented(lambda t: extract_field(model, enc, grid, t, **kw), thresholds, batch,
                                                             connectivity)
            kept = np.flatnonzero(R.keep(labels, sizes, k).reshape(-1)[index])
            cloud = extract_field(model, enc, grid, thr, min_component_nodes=k, connectivity=connectivity, **kw)
            n = cloud.valid()
            assert n == cloud.index.shape[0] == kept.size and 0 < n < index.size
            assert cloud.stage_names == full.stage_names + ("components",) and int(cloud.stage_counts[-1].item()) == n
            assert int(cloud.stage_counts[-2].item()) == index.size
            rows = torch.from_numpy(kept).to(dev)
            assert _rows_equal(cloud, slice(None), full, rows, CLOUD_FIELDS)      # bit for bit: a row is a function of its node
            if case == "fused":
                assert torch.equal(cloud.views, full.views[rows])
            # the largest component of every batch element alone (ties to the smallest label)
            largest = np.flatnonzero(R.keep(labels, sizes, 1, True).reshape(-1)[index])
            only = extract_field(model, enc, grid, thr, largest_only=True, connectivity=connectivity, **kw)
            assert 0 < largest.size < index.size
            assert _rows_equal(only, slice(None), full, torch.from_numpy(largest).to(dev), CLOUD_FIELDS)
            got = cloud_components(only, connectivity=connectivity, batch=batch)
            elements = len(set((index[largest] // grid.num_nodes).tolist()))
            assert len(set(got[0].cpu().tolist())) == int(got[2].item()) == elements
            # both at once: the largest, if it has K nodes
            both = extract_field(model, enc, grid, thr, min_component_nodes=k, largest_only=True, connectivity=connectivity, **kw)
            expect = np.flatnonzero(R.keep(labels, sizes, k, True).reshape(-1)[index])
            assert _rows_equal(both, slice(None), full, torch.from_numpy(expect).to(dev), CLOUD_FIELDS)
            # cloud_components of the unfiltered cloud = the restatement, per row
            got = cloud_components(full, connectivity=connectivity)
            assert np.array_equal(got[0].cpu().numpy(), labels.reshape(-1)[index])
            assert np.array_equal(got[1].cpu().numpy(), sizes.reshape(-1)[index])
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


def test_cloud_components_equals_the_dense_labels_and_honours_a_padded_count(model, dev):
    from neural_jacobian_field_amd.field_volume import cloud_components, dominant_joint, extract_field, label_components
    grid = _grid((17, 13, 11))
    enc = _encoding(2, dev)
    thr, full, labels, sizes, index, _ = _fragmented(lambda t: extract_field(model, enc, grid, t), _thresholds(model, enc, grid), 2)
    labels, sizes = labels.reshape(-1)[index], sizes.reshape(-1)[index]
    n = full.index.shape[0]
    occupancy = torch.zeros(2 * grid.num_nodes, device=dev)
    occupancy[full.index.long()] = 1.0
    for connectivity in R.CONNECTIVITIES:
        dense = label_components(grid, occupancy.reshape(2, -1), 0.5, connectivity=connectivity)
        got = cloud_components(full, connectivity=connectivity)
        assert torch.equal(got[0], dense.labels.reshape(-1)[full.index.long()])
        assert torch.equal(got[1], dense.sizes.reshape(-1)[full.index.long()]) and torch.equal(got[2], dense.count)
    padded = extract_field(model, enc, grid, thr, max_points=n + 37)
    padded.index[n:] = full.index[0]                                  # rows past the count hold anything: they are never read
    got = cloud_components(padded, batch=2)
    assert np.array_equal(got[0][:n].cpu().numpy(), labels) and np.array_equal(got[1][:n].cpu().numpy(), sizes)
    assert (got[0][n:] == -1).all() and (got[1][n:] == 0).all()
    # keyed by the joint that moves a node most: the restatement with the same per-node keys
    keys = dominant_joint(full.jacobian)
    assert keys.dtype == torch.int32 and 0 <= int(keys.min()) and int(keys.max()) < 8
    dense_keys = np.zeros(2 * grid.num_nodes, dtype=np.int32)
    dense_keys[full.index.cpu().numpy()] = keys.cpu().numpy()
    inside = occupancy.cpu().numpy().astype(bool).reshape(2, -1)
    ref = R.label(inside, grid.dims, 6, dense_keys.reshape(2, -1))
    got = cloud_components(full, keys=keys)
    assert np.array_equal(got[0].cpu().numpy(), ref[0].reshape(-1)[index]) and int(got[2].item()) == ref[2]
    assert np.array_equal(got[1].cpu().numpy(), ref[1].reshape(-1)[index])


@pytest.mark.parametrize("views", [1, 2])
def test_extract_mesh_drops_the_surfaces_of_small_components(model, dev, views):
    from neural_jacobian_field_amd.field_volume import extract_mesh, fuse_views, mesh_from_values
    grid = _grid((17, 13, 11))
    enc = _encoding(2, dev)
    batch = 2 // views
    values = _dense_density(model, enc, grid)
    thresholds = _thresholds(model, enc, grid)
    if views == 1:
        comp_valid = _seen(grid, enc, dev)
    else:
        values, _, comp_valid = fuse_views(grid, values, enc, views_per_scene=views)
        comp_valid = comp_valid.cpu().numpy()
    v = values.cpu().numpy()
    kw = dict(views_per_scene=views)
    distinct = []
    for thr in thresholds:
        inside = (v >= np.float32(thr)) & comp_valid
        labels, sizes, count = R.label(inside, grid.dims, 14)
        distinct = sorted(set(sizes[inside].tolist()))
        if len(distinct) >= 2:
            break
    assert len(distinct) >= 2, "no threshold of the list fragments the field"
    k = distinct[len(distinct) // 2]
    dropped = inside & (sizes < k)
    assert dropped.any() and (inside & ~dropped).any()                # the precondition: the filter is not vacuous
    full = extract_mesh(model, enc, grid, thr, **kw)
    mesh = extract_mesh(model, enc, grid, thr, min_component_nodes=k, **kw)
    expect = mesh_from_values(grid, values, thr, valid=torch.from_numpy(comp_valid & ~dropped).to(dev))
    assert mesh.valid() == expect.valid() and mesh.valid()[1] > 0
    assert all(torch.equal(getattr(mesh, f), getattr(expect, f)) for f in MESH_FIELDS)
    assert int(mesh.components_status.item()) == 0
    # a subset of the unfiltered triangles, by cell; what is missing lies in cells that touch a dropped node
    cells_full, cells = full.triangle_cell.cpu().numpy(), mesh.triangle_cell.cpu().numpy()
    assert set(cells.tolist()) <= set(cells_full.tolist()) and cells.size < cells_full.size
    cx, cy, cz = (d - 1 for d in grid.dims)
    touched = np.zeros((batch, cx, cy, cz), dtype=bool)
    d4 = dropped.reshape((batch,) + grid.dims)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                touched |= d4[:, dx:dx + cx, dy:dy + cy, dz:dz + cz]
    count_full, count_kept = np.bincount(cells_full, minlength=touched.size), np.bincount(cells, minlength=touched.size)
    changed = count_full != count_kept
    assert changed.any() and touched.reshape(-1)[changed].all()
    # largest_only: one component per batch element
    only = extract_mesh(model, enc, grid, thr, largest_only=True, **kw)
    keep = R.keep(labels, sizes, 1, True)
    expect = mesh_from_values(grid, values, thr, valid=torch.from_numpy(comp_valid & ~(inside & ~keep)).to(dev))
    assert all(torch.equal(getattr(only, f), getattr(expect, f)) for f in MESH_FIELDS)


def _seen(grid, enc, dev):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import _cameras
    b = enc.extrinsics.shape[0]
    total = b * grid.num_nodes
    idx, count = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    hip.field_select(grid.c_grid(), b, total, idx, count, cams=_cameras(enc, False, action_dim=None))
    inside = np.zeros(total, dtype=bool)
    inside[idx[:int(count.item())].cpu().numpy()] = True
    return inside.reshape(b, grid.num_nodes)


# ---- 6. determinism and capture ------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes(dev):
    from neural_jacobian_field_amd.field_volume import label_components
    grid = _grid(RANDOM)
    values = torch.from_numpy(np.random.default_rng(4).random((2, grid.num_nodes)).astype(np.float32)).to(dev)
    for connectivity in R.CONNECTIVITIES:
        a, b = (label_components(grid, values, 0.55, connectivity=connectivity) for _ in range(2))
        assert torch.equal(a.labels, b.labels) and torch.equal(a.sizes, b.sizes) and torch.equal(a.count, b.count)


def test_the_capacity_forms_replay_to_the_eager_bytes(model, dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import extract_field, extract_mesh
    grid = _grid((17, 13, 11))
    enc = _encoding(2, dev)
    thr, full, _, _, _, k = _fragmented(lambda t: extract_field(model, enc, grid, t), _thresholds(model, enc, grid), 2)
    enc2 = PixelEncoding(features=synthetic.synthetic_features(2, IMG, IMG, seed=9).to(dev), extrinsics=enc.extrinsics,
                         intrinsics=enc.intrinsics, action=None)
    kw = dict(min_component_nodes=k)
    eager, eager2 = extract_field(model, enc, grid, thr, **kw), extract_field(model, enc2, grid, thr, **kw)
    n, n2 = eager.valid(), eager2.valid()
    assert n > 0 and n2 > 0
    again = extract_field(model, enc, grid, thr, **kw)
    assert _rows_equal(eager, slice(None), again, slice(None), CLOUD_FIELDS)
    short = extract_field(model, enc, grid, thr, max_points=max(n - 3, 1), **kw)
    assert int(short.count.item()) == n and _rows_equal(short, slice(0, short.valid()), eager, slice(0, short.valid()), CLOUD_FIELDS)
    mesh_eager2 = extract_mesh(model, enc2, grid, thr, **kw)
    v2, t2 = mesh_eager2.valid()
    static = PixelEncoding(features=enc.features.clone(), extrinsics=enc.extrinsics, intrinsics=enc.intrinsics, action=None)
    v1, t1 = extract_mesh(model, enc, grid, thr, **kw).valid()
    assert v2 > 0 and t2 > 0
    caps = dict(max_vertices=max(v1, v2) + 50, max_triangles=max(t1, t2) + 50)
    cap = max(n, n2) + 31
    extract_field(model, static, grid, thr, max_points=cap, **kw)                # eager warm-ups
    extract_mesh(model, static, grid, thr, **caps, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cloud = extract_field(model, static, grid, thr, max_points=cap, **kw)
        mesh = extract_mesh(model, static, grid, thr, **caps, **kw)
    static.features.copy_(enc2.features)
    graph.replay()
    torch.cuda.synchronize()
    assert cloud.valid() == n2 and int(cloud.components_status.item()) == 0 and int(mesh.components_status.item()) == 0
    assert cloud.stage_names[-1] == "components"
    assert _rows_equal(cloud, slice(0, n2), eager2, slice(0, n2), CLOUD_FIELDS)
    assert mesh.valid() == (v2, t2)
    for f in MESH_FIELDS + ("color", "jacobian"):
        rows = t2 if f.startswith("tri") else v2
        assert torch.equal(getattr(mesh, f)[:rows], getattr(mesh_eager2, f)[:rows]), f
