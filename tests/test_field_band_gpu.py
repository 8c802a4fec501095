"""GPU tests of the coarse-to-fine band (field_volume.band_from_values / band_leaks, the ``coarse`` / ``coarse_threshold`` /
``coarse_dilate`` keywords of extract_field / extract_mesh; njf_field_band / njf_field_scatter / njf_field_band_leaks; DESIGN.md
section 14).

Everything is exact equality: ``block_active``, ``band``, ``index``, ``count`` and the leak count with the numpy restatement of
the semantics (tests/field_band_restatement.py); the banded extractions bit for bit with the dense ones in which the nodes
outside the restated band are invalid.  Two batch elements (or scenes) throughout, so the batch boundary falls inside a
workgroup.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import block_offsets_cases as K
import field_band_restatement as R
import field_components_restatement as RC

pytestmark = pytest.mark.gpu

IMG = 64
CRAFTED = (9, 13, 17)    # k = 4: m = (2, 3, 4), 60 coarse nodes and 24 blocks, 1,989 nodes per element: two workgroups
LARGE = (17, 25, 33)     # k = 8: m = (2, 3, 4), 14,025 nodes per element
SCENE = (17, 13, 9)      # the synthetic model's grid: 1,989 nodes per element
CLOUD_FIELDS = ("index", "xyz", "density", "color", "jacobian")
MESH_FIELDS = ("vertex_node", "vertex_edge", "triangles", "triangle_cell", "vertex_t", "vertices")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _grid(dims):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), dims)


def _coarse_nodes(dims, k):
    m = R.blocks_per_axis(dims, k)
    return (m[0] + 1) * (m[1] + 1) * (m[2] + 1)


def _band(dev, dims, k, values, threshold, valid=None, d=1, max_nodes=None):
    from neural_jacobian_field_amd.field_volume import band_from_values
    band = band_from_values(_grid(dims), k, torch.from_numpy(values).to(dev), threshold, dilate=d, max_nodes=max_nodes,
                            coarse_valid=None if valid is None else torch.from_numpy(valid).to(dev))
    assert band.block_active.dtype == band.band.dtype == torch.uint8 and band.index.dtype == band.count.dtype == torch.int32
    m = R.blocks_per_axis(dims, k)
    assert tuple(band.block_active.shape) == (values.shape[0], m[0] * m[1] * m[2])
    assert tuple(band.band.shape) == (values.shape[0], dims[0] * dims[1] * dims[2]) and band.count.shape == (1,)
    assert band.coarse_grid.dims == tuple(mc + 1 for mc in m)
    return band


def _assert_equals_restatement(dev, dims, k, values, threshold, valid=None, d=1):
    band = _band(dev, dims, k, values, threshold, valid, d)
    active, in_band, index, count = R.full(values, valid, threshold, dims, k, d)
    assert np.array_equal(band.block_active.cpu().numpy(), active.astype(np.uint8)), ("block_active", dims, k, d)
    assert np.array_equal(band.band.cpu().numpy(), in_band.astype(np.uint8)), ("band", dims, k, d)
    assert int(band.count.item()) == count and band.index.shape[0] == count
    assert np.array_equal(band.index.cpu().numpy().astype(np.int64), index), ("index", dims, k, d)
    return band, active, in_band


# ---- 1. band_from_values against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,k", [(CRAFTED, 4), (LARGE, 8), ((5, 5, 5), 2), ((5, 5, 5), 4)])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_band_from_values_equals_the_restatement(dev, dims, k, d):
    rng = np.random.default_rng(100 * k + d)
    values = rng.random((2, _coarse_nodes(dims, k))).astype(np.float32)
    valid = rng.random(values.shape) < 0.8
    _assert_equals_restatement(dev, dims, k, values, 0.9, None, d)
    _assert_equals_restatement(dev, dims, k, values, 0.85, valid, d)
    _assert_equals_restatement(dev, dims, k, values, 0.85, valid.astype(np.uint8), d)


@pytest.mark.parametrize("dims,batch,kind,d", K.BAND_CASES)
def test_band_past_256_workgroups_equals_the_restatement(dev, dims, batch, kind, d):
    """The band's list with two sums per thread of the one-workgroup scan of its offsets: 302 workgroups at 65 x 65 x 73, 305 at
    two elements of 49 x 49 x 65 (k = 8).  "late": hits only on the last coarse x layer of the last element -- every offset in
    front of workgroup 256 is zero, the first that is not belongs to a run past it (tests/test_block_primitives_cpu.py)."""
    values = K.band_values(dims, batch, kind)
    band, _, in_band = _assert_equals_restatement(dev, dims, K.BAND_FACTOR, values, K.BAND_THRESHOLD, None, d)
    nodes = batch * dims[0] * dims[1] * dims[2]
    blocks = K.workgroups(nodes, K.BAND_BLOCK)
    filled = np.flatnonzero(K.block_sums(in_band.reshape(-1), K.BAND_BLOCK))
    print(f"workgroups {blocks}, per {K.per_thread(blocks)}, survivors {int(band.count.item())} of {nodes}, in {filled.size} workgroups "
          f"({filled[0]} .. {filled[-1]})")
    assert blocks > K.THREADS and 0 < int(band.count.item()) < nodes
    assert kind != "late" or filled[0] >= K.THREADS


@pytest.mark.parametrize("share", [0.05, 0.5])
@pytest.mark.parametrize("dims,k", [(CRAFTED, 4), (LARGE, 8), (LARGE, 2)])
def test_random_occupancy_and_its_leaks_equal_the_restatement(dev, dims, k, share):
    from neural_jacobian_field_amd.field_volume import band_leaks
    rng = np.random.default_rng(int(100 * share) + k)
    hit = rng.random((2, _coarse_nodes(dims, k))) < share
    for d in (0, 1):
        band, _, in_band = _assert_equals_restatement(dev, dims, k, hit.astype(np.float32), 0.5, None, d)
        inside = in_band & (rng.random(in_band.shape) < 0.3)
        index = torch.from_numpy(R.band_list(inside).astype(np.int32)).to(dev)
        expect = R.leaks(inside, in_band, dims)
        assert int(band_leaks(_grid(dims), band.band, index).item()) == expect
        # a device count below the list's length: the rows past it are never read
        padded = torch.cat([index, torch.full((50,), 2 ** 31 - 1, dtype=torch.int32, device=dev)])
        count = torch.tensor([index.shape[0]], dtype=torch.int32, device=dev)
        assert int(band_leaks(_grid(dims), band.band.to(torch.bool), padded, count).item()) == expect
        if share < 0.1 and d == 0 and k != 2:
            assert 0 < expect < inside.sum()


# ---- 2. crafted cases ------------------------------------------------------------------------------------------------------------
def _coarse_index(dims, k, qx, qy, qz):
    m = R.blocks_per_axis(dims, k)
    return (qx * (m[1] + 1) + qy) * (m[2] + 1) + qz


def test_a_single_hit_at_a_corner_on_a_face_and_at_a_shared_block_corner(dev):
    dims, k = CRAFTED, 4
    nodes = dims[0] * dims[1] * dims[2]
    m = R.blocks_per_axis(dims, k)
    for where, own, dilated in (((0, 0, 0), 1, 8), ((0, 1, 2), 4, 2 * 3 * 4), ((1, 2, 2), 8, 2 * 3 * 4), ((2, 3, 4), 1, 8)):
        values = np.zeros((2, _coarse_nodes(dims, k)), dtype=np.float32)
        values[0, _coarse_index(dims, k, *where)] = 1.0
        for d in (0, 1, 2):
            # hit q activates the blocks j with q - 1 - d <= j_c <= q + d, clipped to [0, m_c - 1]
            blocks = int(np.prod([min(q + d, mc - 1) - max(q - 1 - d, 0) + 1 for q, mc in zip(where, m)]))
            assert d == 2 or blocks == (own, dilated)[d]
            band, active, in_band = _assert_equals_restatement(dev, dims, k, values, 0.5, None, d)
            assert active[0].sum() == blocks, (where, d)                     # the dilation is clipped at the grid faces
            assert not active[1].any() and not in_band[1].any()              # a hit in element 0 activates nothing in element 1
            assert int(band.index.max().item()) < nodes
    # the node of the hit itself is in the band, and with d = 0 so are exactly the nodes within k of it along every axis
    values = np.zeros((2, _coarse_nodes(dims, k)), dtype=np.float32)
    values[1, _coarse_index(dims, k, 1, 2, 2)] = 1.0
    _, _, in_band = _assert_equals_restatement(dev, dims, k, values, 0.5, None, 0)
    cube = np.zeros(dims, dtype=bool)
    cube[0:9, 4:13, 4:13] = True
    assert np.array_equal(in_band[1].reshape(dims), cube) and not in_band[0].any()


def test_special_values_the_threshold_itself_and_the_valid_mask(dev):
    dims, k = CRAFTED, 4
    thr = np.float32(0.25)
    values = np.full((2, _coarse_nodes(dims, k)), thr - np.spacing(thr), dtype=np.float32)    # just below: no hit
    q = [_coarse_index(dims, k, *w) for w in ((0, 0, 0), (2, 0, 0), (0, 3, 0), (2, 3, 4), (0, 0, 4))]
    values[0, q[0]] = np.nan
    values[0, q[1]] = -np.inf
    values[0, q[2]] = np.inf
    values[1, q[3]] = thr                                                     # equal to the threshold: a hit
    values[1, q[4]] = np.nan
    hit = R.hits(values, thr)
    assert hit.sum() == 2 and hit[0, q[2]] and hit[1, q[3]]
    _, active, _ = _assert_equals_restatement(dev, dims, k, values, float(thr), None, 0)
    assert active[0].sum() == 1 and active[1].sum() == 1
    _assert_equals_restatement(dev, dims, k, values, float(thr), None, 1)
    valid = np.ones(values.shape, dtype=bool)
    valid[0, q[2]] = False                                                    # the mask removes the hit of element 0
    band, active, _ = _assert_equals_restatement(dev, dims, k, values, float(thr), valid, 1)
    assert not active[0].any() and active[1].any()
    assert int(band.index.min().item()) >= dims[0] * dims[1] * dims[2]


def test_all_hit_none_hit_and_the_empty_list_downstream(dev):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import band_leaks, label_components, mesh_from_values
    dims, k = CRAFTED, 4
    grid, nodes = _grid(dims), dims[0] * dims[1] * dims[2]
    ones = np.ones((2, _coarse_nodes(dims, k)), dtype=np.float32)
    for d in (0, 2):
        band, _, _ = _assert_equals_restatement(dev, dims, k, ones, 0.5, None, d)
        assert int(band.count.item()) == 2 * nodes and torch.equal(band.index, torch.arange(2 * nodes, dtype=torch.int32, device=dev))
        assert int(band_leaks(grid, band.band, band.index).item()) == 0
        band, _, _ = _assert_equals_restatement(dev, dims, k, ones, 1.5, None, d)
        assert int(band.count.item()) == 0 and band.index.shape == (0,) and not band.band.any() and not band.block_active.any()
    # downstream of an empty band: every call still returns an empty result
    assert int(band_leaks(grid, band.band, band.index).item()) == 0
    values = torch.rand(2, nodes, device=dev)
    mesh = mesh_from_values(grid, values, 0.5, valid=band.band)
    assert mesh.valid() == (0, 0) and mesh.vertices.shape == (0, 3)
    assert int(label_components(grid, values, 0.5, valid=band.band).count.item()) == 0
    out = torch.zeros(7, device=dev)
    hip.field_scatter(torch.empty(0, device=dev), band.index, None, 0, out)
    assert not out.any()


def test_two_calls_give_equal_bytes_and_the_capacity_form_keeps_the_first_rows(dev):
    dims, k = LARGE, 8
    values = np.random.default_rng(21).random((2, _coarse_nodes(dims, k))).astype(np.float32)
    a, b = (_band(dev, dims, k, values, 0.9, d=0) for _ in range(2))
    for f in ("block_active", "band", "index", "count"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    n = int(a.count.item())
    assert 1000 < n < 2 * dims[0] * dims[1] * dims[2]
    short = _band(dev, dims, k, values, 0.9, d=0, max_nodes=n - 123)
    assert int(short.count.item()) == n and short.index.shape == (n - 123,) and torch.equal(short.index, a.index[:n - 123])
    assert torch.equal(short.band, a.band) and torch.equal(short.block_active, a.block_active)
    padded = _band(dev, dims, k, values, 0.9, d=0, max_nodes=n + 77)
    assert int(padded.count.item()) == n and padded.index.shape == (n + 77,) and torch.equal(padded.index[:n], a.index)


def test_field_scatter_reads_its_count_on_the_device_and_skips_indices_outside(dev):
    from neural_jacobian_field_amd import hip
    rng = np.random.default_rng(8)
    size, capacity, used = 5000, 3000, 1531                                  # twelve workgroups, the count inside the sixth
    at = np.sort(rng.choice(size, used, replace=False)).astype(np.int32)
    at[[3, 700]] = [-5, size]                                                 # two entries outside [0, size): skipped
    indices = np.concatenate([at, rng.choice([-1, size, 2 ** 31 - 1, 17], capacity - used)]).astype(np.int32)
    values = rng.random(capacity).astype(np.float32)
    values[used:] = np.nan                                                    # rows past the count: poisoned
    expect = np.full(size, -2.0, dtype=np.float32)
    keep = (at >= 0) & (at < size)
    expect[at[keep]] = values[:used][keep]
    out = torch.full((size,), -2.0, device=dev)
    hip.field_scatter(torch.from_numpy(values).to(dev), torch.from_numpy(indices).to(dev),
                      torch.tensor([used], dtype=torch.int32, device=dev), capacity, out)
    assert np.array_equal(out.cpu().numpy(), expect)
    # a count above the capacity is clamped to it; without a count every row is used
    out = torch.full((size,), -2.0, device=dev)
    hip.field_scatter(torch.from_numpy(values).to(dev), torch.from_numpy(indices).to(dev),
                      torch.tensor([capacity + 9], dtype=torch.int32, device=dev), used, out)
    assert np.array_equal(out.cpu().numpy(), expect)
    out = torch.full((size,), -2.0, device=dev)
    hip.field_scatter(torch.from_numpy(values).to(dev), torch.from_numpy(indices).to(dev), None, used, out)
    assert np.array_equal(out.cpu().numpy(), expect)


def test_a_blob_strictly_inside_the_band_does_not_leak(dev):
    from neural_jacobian_field_amd.field_volume import band_leaks
    dims, k = LARGE, 8
    values = np.zeros((2, _coarse_nodes(dims, k)), dtype=np.float32)
    values[1, _coarse_index(dims, k, 1, 1, 2)] = 1.0
    band, _, in_band = _assert_equals_restatement(dev, dims, k, values, 0.5, None, 0)      # nodes [0..16] x [0..16] x [8..24]
    blob = np.zeros((2,) + dims, dtype=bool)
    blob[1, 1:16, 1:16, 9:24] = True                                          # one node away from every band face inside the grid
    blob[1, 0, 5, 12] = blob[1, 16, 0, 20] = True                             # on grid faces: nothing beyond to leak to
    index = torch.from_numpy(R.band_list(blob).astype(np.int32)).to(dev)
    assert R.leaks(blob.reshape(2, -1), in_band, dims) == 0 and int(band_leaks(_grid(dims), band.band, index).item()) == 0
    blob[1, 8, 16, 12] = True                                                 # on the band's face y = 16: its +y neighbours are outside
    index = torch.from_numpy(R.band_list(blob).astype(np.int32)).to(dev)
    assert R.leaks(blob.reshape(2, -1), in_band, dims) == 1 and int(band_leaks(_grid(dims), band.band, index).item()) == 1


# ---- 3. the extractions on the synthetic model -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model
    cache = {}

    def get(kind="jacobian_mlp", adim=8):
        if (kind, adim) not in cache:
            cfg = model_cfg_from_dict({"action_dim": adim, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                                       "action_decoder": {"name": kind}})
            model = Model(cfg)
            model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes(kind, adim), seed=0), strict=True)
            cache[(kind, adim)] = model.to(dev).eval().requires_grad_(False)
        return cache[(kind, adim)]

    return get


def _encoding(batch, dev, adim=8, seed=1):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    c2w = synthetic.general_pose(7, batch, scale=0.04)
    c2w[0] = torch.eye(4)
    k = synthetic.synthetic_cameras(batch)["ctxt_k_norm"]
    return PixelEncoding(features=synthetic.synthetic_features(batch, IMG, IMG, seed=seed).to(dev), extrinsics=c2w.to(dev),
                         intrinsics=k.to(dev), action=synthetic.synthetic_action(batch, adim).to(dev))


def _dense_density(model, enc, grid):
    b = enc.extrinsics.shape[0]
    xyz = grid.points(device=enc.extrinsics.device)
    head, _ = model.compute_density(xyz[None].expand(b, -1, 3).contiguous(), enc)
    return head.density.reshape(b, grid.num_nodes).clone()


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


def _at_coarse_nodes(per_node, dims, k):
    """[B, N] -> [B, M]: coarse node j is fine node k*j."""
    b = per_node.shape[0]
    return np.ascontiguousarray(per_node.reshape((b,) + tuple(dims))[:, ::k, ::k, ::k]).reshape(b, -1)


def _partial_band(values, valid, dims):
    """(k, d, coarse threshold, restated band [B, N]) with a band share between 10 % and 60 %: the coarse threshold is a
    quantile of the dense values, the first of a fixed list of (k, d, quantile) that lands in the range."""
    finite = values[np.isfinite(values)].astype(np.float64)
    for k, d in ((4, 0), (2, 1), (2, 0), (4, 1)):
        for q in (0.97, 0.93, 0.88, 0.99, 0.8, 0.995, 0.7):
            thr = float(np.float32(np.quantile(finite, q)))
            cvalid = None if valid is None else _at_coarse_nodes(valid, dims, k)
            in_band = R.full(_at_coarse_nodes(values, dims, k), cvalid, thr, dims, k, d)[1]
            if 0.1 <= in_band.mean() <= 0.6:
                print(f"partial band: k = {k}, d = {d}, quantile {q}, share {in_band.mean():.3f}")
                return k, d, thr, in_band
    raise AssertionError("no (k, d, quantile) of the list gives a band share between 10 % and 60 %")


def _mesh_equal(a, b, fields=MESH_FIELDS):
    return a.valid() == b.valid() and all(torch.equal(getattr(a, f), getattr(b, f)) for f in fields)


def _points_forward_rows(model, enc, mesh):
    """hip.points_forward on the returned vertex positions, per batch element, padded to the largest one -> rows [V, ...]."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import _cameras, _map_of
    dec = model.decoder
    dev = mesh.vertices.device
    b = enc.extrinsics.shape[0]
    which = mesh.batch_index.long()
    counts = torch.bincount(which, minlength=b)
    pad = max(int(counts.max()), 1)
    xyz = torch.zeros(b, pad, 3, device=dev)
    xyz[:, :, 2] = 1.5
    slot = torch.arange(which.numel(), device=dev) - torch.cumsum(counts, 0)[which] + counts[which]
    xyz[which, slot] = mesh.vertices
    cams = _cameras(enc, False, action_dim=dec.kernel_action_dim)
    w, bd, bc, bj = dec.packed()
    gmap, base = _map_of(dec, enc.features)
    a_dim = dec.kernel_action_dim
    color = torch.empty(b * pad, 3, device=dev)
    jac = torch.empty(b * pad, 3 * a_dim, device=dev)
    hip.points_forward(xyz, None, cams, hip.make_feature_map(gmap), base + dec.GOFF_DENSITY, base + dec.GOFF_JACOBIAN, 1, w, bd,
                       b_color=bc, b_jacobian=bj, jacobian_kind=dec.JACOBIAN_KIND, color=color, jacobian=jac,
                       precision=dec.precision, jacobian_precision=dec.j_precision)
    rows = which * pad + slot
    return color[rows], jac[rows].reshape(-1, a_dim, 3)


@pytest.mark.parametrize("precision", ["f32", None])
@pytest.mark.parametrize("kind,adim", [("jacobian_mlp", 8), ("jacobian_transformer", 6)])
def test_a_band_that_holds_every_node_changes_nothing(models, dev, kind, adim, precision):
    """(a) coarse_threshold = 0: the densities are trunc_exp outputs, every finite coarse node hits and the band is the grid --
    the list, the scatter and the valid plumbing lose nothing."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import extract_field, extract_mesh
    model = models(kind, adim)
    model.set_precision(hip.DEFAULT_PRECISION if precision is None else precision)
    try:
        grid, enc = _grid(SCENE), _encoding(2, dev, adim)
        thr = float(torch.quantile(_dense_density(model, enc, grid).double().reshape(-1), 0.6))
        for in_frustum in (True, False):
            dense = extract_mesh(model, enc, grid, thr, in_frustum=in_frustum)
            mesh = extract_mesh(model, enc, grid, thr, in_frustum=in_frustum, coarse=4, coarse_threshold=0.0)
            assert int(mesh.band_count.item()) == 2 * grid.num_nodes
            assert dense.valid()[1] > 0 and _mesh_equal(mesh, dense, MESH_FIELDS + ("color", "jacobian"))
            if not in_frustum:
                assert int(mesh.band_leaks.item()) == 0
            full = extract_field(model, enc, grid, thr, in_frustum=in_frustum)
            cloud = extract_field(model, enc, grid, thr, in_frustum=in_frustum, coarse=4, coarse_threshold=0.0)
            assert int(cloud.band_count.item()) == 2 * grid.num_nodes and int(cloud.band_leaks.item()) == 0
            assert full.valid() > 0 and all(torch.equal(getattr(cloud, f), getattr(full, f)) for f in CLOUD_FIELDS)
            assert cloud.stage_names == ("band",) + full.stage_names
            assert [int(c.item()) for c in cloud.stage_counts[1:]] == [int(c.item()) for c in full.stage_counts]
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


@pytest.mark.parametrize("precision", ["f32", None])
def test_a_partial_band_equals_the_dense_route_with_the_band_as_valid_mask(models, dev, precision):
    """(b) in_frustum = False: the mesh is mesh_from_values(dense values, valid = restated band), its attributes are
    njf_points_forward on the vertices, the cloud is the rows of the dense cloud inside the restated band."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import extract_field, extract_mesh, mesh_from_values
    model = models()
    model.set_precision(hip.DEFAULT_PRECISION if precision is None else precision)
    try:
        grid, enc = _grid(SCENE), _encoding(2, dev)
        density = _dense_density(model, enc, grid)
        values = density.cpu().numpy()
        thr = float(torch.quantile(density.double().reshape(-1), 0.6))
        k, d, coarse_thr, in_band = _partial_band(values, None, SCENE)
        kw = dict(in_frustum=False, coarse=k, coarse_threshold=coarse_thr, coarse_dilate=d)
        mesh = extract_mesh(model, enc, grid, thr, **kw)
        expect = mesh_from_values(grid, density, thr, valid=torch.from_numpy(in_band).to(dev))
        whole = mesh_from_values(grid, density, thr)
        assert 0 < expect.valid()[1] < whole.valid()[1]                       # the band cuts the surface: the mask is not vacuous
        assert _mesh_equal(mesh, expect)
        color, jacobian = _points_forward_rows(model, enc, mesh)
        assert torch.equal(mesh.color, color) and torch.equal(mesh.jacobian, jacobian)
        assert int(mesh.band_count.item()) == in_band.sum()
        inside = (values >= np.float32(thr)) & in_band
        leaks = R.leaks(inside, in_band, SCENE)
        assert int(mesh.band_leaks.item()) == leaks and leaks > 0
        full = extract_field(model, enc, grid, thr, in_frustum=False)
        cloud = extract_field(model, enc, grid, thr, **kw)
        rows = torch.from_numpy(np.flatnonzero(in_band.reshape(-1)[full.index.cpu().numpy()])).to(dev)
        assert 0 < rows.numel() < full.index.shape[0] == full.valid()
        assert cloud.valid() == cloud.index.shape[0] == rows.numel()
        assert all(torch.equal(getattr(cloud, f), getattr(full, f)[rows]) for f in CLOUD_FIELDS)
        assert int(cloud.band_leaks.item()) == leaks and int(cloud.band_count.item()) == in_band.sum()
        assert cloud.stage_names == ("band", "density") and int(cloud.stage_counts[0].item()) == in_band.sum()
        # with the frustum and the proposal cull in front, the band is one more predicate
        seen = _seen(grid, enc, dev)
        full = extract_field(model, enc, grid, thr, cull=0.0)
        cloud = extract_field(model, enc, grid, thr, cull=0.0, **dict(kw, in_frustum=True))
        rows = torch.from_numpy(np.flatnonzero(in_band.reshape(-1)[full.index.cpu().numpy()])).to(dev)
        assert all(torch.equal(getattr(cloud, f), getattr(full, f)[rows]) for f in CLOUD_FIELDS)
        assert cloud.stage_names == ("band", "frustum", "proposal", "density")
        assert int(cloud.band_leaks.item()) == R.leaks(inside & seen, in_band, SCENE)
        mesh = extract_mesh(model, enc, grid, thr, **dict(kw, in_frustum=True))
        assert _mesh_equal(mesh, mesh_from_values(grid, density, thr, valid=torch.from_numpy(in_band & seen).to(dev)))
        assert int(mesh.band_leaks.item()) == R.leaks(inside & seen, in_band, SCENE)
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


@pytest.mark.parametrize("mode", ["mean", "min"])
@pytest.mark.parametrize("in_frustum", [False, True])
def test_scenes_of_two_views(models, dev, mode, in_frustum):
    """(c) views_per_scene = 2 (B = 4, G = 2): both comparisons against the fused dense route."""
    from neural_jacobian_field_amd.field_volume import extract_field, extract_mesh, fuse_views, mesh_from_values
    model = models()
    grid, enc = _grid(SCENE), _encoding(4, dev)
    fuse = dict(views_per_scene=2, fuse=mode)
    fused, _, valid = fuse_views(grid, _dense_density(model, enc, grid), enc if in_frustum else None, views_per_scene=2, mode=mode)
    values, ok = fused.cpu().numpy(), valid.cpu().numpy()
    thr = float(torch.quantile(fused[valid].double(), 0.6))
    dense_mesh = extract_mesh(model, enc, grid, thr, in_frustum=in_frustum, **fuse)
    dense_cloud = extract_field(model, enc, grid, thr, in_frustum=in_frustum, **fuse)
    assert dense_mesh.valid()[1] > 0 and dense_cloud.valid() > 0
    # the whole grid as band: here the fused density may be exactly 0, so the share is asserted, not assumed
    everything = R.full(_at_coarse_nodes(values, SCENE, 4), _at_coarse_nodes(ok, SCENE, 4), 0.0, SCENE, 4, 1)[1]
    mesh = extract_mesh(model, enc, grid, thr, in_frustum=in_frustum, coarse=4, coarse_threshold=0.0, **fuse)
    cloud = extract_field(model, enc, grid, thr, in_frustum=in_frustum, coarse=4, coarse_threshold=0.0, **fuse)
    assert int(mesh.band_count.item()) == int(cloud.band_count.item()) == everything.sum()
    if not in_frustum:
        assert everything.all()
    if everything.all():
        assert _mesh_equal(mesh, dense_mesh, MESH_FIELDS + ("color", "jacobian", "vertex_views"))
        assert all(torch.equal(getattr(cloud, f), getattr(dense_cloud, f)) for f in CLOUD_FIELDS + ("views",))
    # a partial band
    k, d, coarse_thr, in_band = _partial_band(np.where(ok, values, -np.inf), ok, SCENE)
    kw = dict(in_frustum=in_frustum, coarse=k, coarse_threshold=coarse_thr, coarse_dilate=d, **fuse)
    mesh = extract_mesh(model, enc, grid, thr, **kw)
    expect = mesh_from_values(grid, fused, thr, valid=torch.from_numpy(ok & in_band).to(dev))
    assert 0 < expect.valid()[1] < dense_mesh.valid()[1] and _mesh_equal(mesh, expect)
    inside = (values >= np.float32(thr)) & ok & in_band
    leaks = R.leaks(inside, in_band, SCENE)
    assert int(mesh.band_leaks.item()) == leaks and int(mesh.band_count.item()) == in_band.sum()
    # colour, Jacobian and the view mask of a vertex are functions of the vertex alone: those of the dense mesh's equal vertex
    key = lambda m: (m.vertex_node.long() * 8 + m.vertex_edge.long())
    at = torch.searchsorted(key(dense_mesh), key(mesh))
    assert torch.equal(key(dense_mesh)[at], key(mesh))
    for f in ("color", "jacobian", "vertex_views"):
        assert torch.equal(getattr(mesh, f), getattr(dense_mesh, f)[at]), f
    cloud = extract_field(model, enc, grid, thr, **kw)
    rows = torch.from_numpy(np.flatnonzero(in_band.reshape(-1)[dense_cloud.index.cpu().numpy()])).to(dev)
    assert 0 < rows.numel() < dense_cloud.valid() and cloud.valid() == cloud.index.shape[0] == rows.numel()
    assert all(torch.equal(getattr(cloud, f), getattr(dense_cloud, f)[rows]) for f in CLOUD_FIELDS + ("views",))
    assert int(cloud.band_leaks.item()) == leaks and cloud.stage_names == ("band", "density")


@pytest.mark.parametrize("views", [1, 2])
def test_the_component_filter_sees_the_band_as_one_more_valid_mask(models, dev, views):
    """(d) min_component_nodes with coarse: the components are those of the in-band inside nodes."""
    from neural_jacobian_field_amd.field_volume import extract_field, extract_mesh, fuse_views, mesh_from_values
    model = models()
    grid, enc = _grid(SCENE), _encoding(2 * views, dev)
    density = _dense_density(model, enc, grid)
    fuse = dict(views_per_scene=views)
    if views == 1:
        ok = _seen(grid, enc, dev)
    else:
        density, _, valid = fuse_views(grid, density, enc, views_per_scene=views)
        ok = valid.cpu().numpy()
    values = density.cpu().numpy()
    k, d, coarse_thr, in_band = _partial_band(np.where(ok, values, -np.inf) if views > 1 else values, ok if views > 1 else None, SCENE)
    kw = dict(coarse=k, coarse_threshold=coarse_thr, coarse_dilate=d, **fuse)
    done = 0
    for q in (0.6, 0.75, 0.45, 0.85, 0.3):
        thr = float(np.float32(np.quantile(values[ok].astype(np.float64), q)))
        inside = (values >= np.float32(thr)) & ok & in_band
        for connectivity in (14, 6):
            labels, sizes, _ = RC.label(inside, SCENE, connectivity)
            distinct = sorted(set(sizes[inside].tolist()))
            if len(distinct) < 2:
                continue
            n = distinct[len(distinct) // 2]
            dropped = inside & (sizes < n)
            assert dropped.any() and (inside & ~dropped).any()                # the filter is not vacuous
            if connectivity == 14:
                mesh = extract_mesh(model, enc, grid, thr, min_component_nodes=n, **kw)
                expect = mesh_from_values(grid, density, thr, valid=torch.from_numpy(ok & in_band & ~dropped).to(dev))
                assert expect.valid()[1] > 0 and _mesh_equal(mesh, expect) and int(mesh.components_status.item()) == 0
            full = extract_field(model, enc, grid, thr, **fuse)
            cloud = extract_field(model, enc, grid, thr, min_component_nodes=n, connectivity=connectivity, **kw)
            rows = torch.from_numpy(np.flatnonzero((inside & ~dropped).reshape(-1)[full.index.cpu().numpy()])).to(dev)
            assert 0 < rows.numel() == cloud.valid() == cloud.index.shape[0]
            assert all(torch.equal(getattr(cloud, f), getattr(full, f)[rows]) for f in CLOUD_FIELDS)
            assert cloud.stage_names[0] == "band" and cloud.stage_names[-1] == "components"
            assert int(cloud.band_leaks.item()) == R.leaks(inside, in_band, SCENE)
            done += 1
        if done >= 2:
            break
    assert done >= 2, "no threshold of the list fragments the banded field"


@pytest.mark.parametrize("views", [1, 2])
def test_the_capacity_forms_replay_to_the_eager_bytes(models, dev, views):
    """(e) max_points / max_vertices + max_triangles with coarse: no host read, captured after one eager call and replayed on
    a second image's features."""
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import extract_field, extract_mesh
    model = models()
    grid, enc = _grid(SCENE), _encoding(2 * views, dev)
    density = _dense_density(model, enc, grid)
    thr = float(torch.quantile(density.double().reshape(-1), 0.6))
    k, d, coarse_thr, _ = _partial_band(density.cpu().numpy(), None, SCENE)
    kw = dict(coarse=k, coarse_threshold=coarse_thr, coarse_dilate=d, views_per_scene=views)
    enc2 = PixelEncoding(features=synthetic.synthetic_features(2 * views, IMG, IMG, seed=9).to(dev), extrinsics=enc.extrinsics,
                         intrinsics=enc.intrinsics, action=None)
    eager, eager2 = extract_field(model, enc, grid, thr, **kw), extract_field(model, enc2, grid, thr, **kw)
    mesh_eager, mesh_eager2 = extract_mesh(model, enc, grid, thr, **kw), extract_mesh(model, enc2, grid, thr, **kw)
    n, n2 = eager.valid(), eager2.valid()
    (v1, t1), (v2, t2) = mesh_eager.valid(), mesh_eager2.valid()
    assert n > 3 and n2 > 0 and v2 > 0 and t2 > 0
    assert int(eager.band_count.item()) != int(eager2.band_count.item()) or n != n2      # the second image differs
    short = extract_field(model, enc, grid, thr, max_points=n - 3, **kw)
    assert int(short.count.item()) == n and short.index.shape == (n - 3,)
    assert all(torch.equal(getattr(short, f), getattr(eager, f)[:n - 3]) for f in CLOUD_FIELDS)
    assert torch.equal(short.band_leaks, eager.band_leaks) and torch.equal(short.band_count, eager.band_count)
    static = PixelEncoding(features=enc.features.clone(), extrinsics=enc.extrinsics, intrinsics=enc.intrinsics, action=None)
    cap = max(n, n2) + 31
    caps = dict(max_vertices=max(v1, v2) + 50, max_triangles=max(t1, t2) + 50)
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
    assert cloud.valid() == n2 and cloud.index.shape == (cap,)
    assert all(torch.equal(getattr(cloud, f)[:n2], getattr(eager2, f)) for f in CLOUD_FIELDS)
    assert torch.equal(cloud.band_count, eager2.band_count) and torch.equal(cloud.band_leaks, eager2.band_leaks)
    assert mesh.valid() == (v2, t2)
    for f in MESH_FIELDS + ("color", "jacobian"):
        rows = t2 if f.startswith("tri") else v2
        assert torch.equal(getattr(mesh, f)[:rows], getattr(mesh_eager2, f)[:rows]), f
    assert torch.equal(mesh.band_count, mesh_eager2.band_count) and torch.equal(mesh.band_leaks, mesh_eager2.band_leaks)
