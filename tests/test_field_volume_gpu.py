"""GPU tests of the voxel-grid field extraction (field_volume.py; njf_field_points / njf_field_select / njf_field_forward).

Every comparison is against the EXISTING dense route on the same floats: ``grid.points()`` fed to ``Model.compute_density``
(density, Jacobian), ``decoder.forward`` (colour) and ``DensityDecoderMlp.get_density`` (proposal density), then the
predicates in torch (``>=``, ``nonzero``, gather).  The dense route is never the code under test.

Band rule (both thresholds): a node whose dense value lies within 1e-4 x threshold of the threshold may fall on either side;
such nodes may be at most 1 % of the dense set -- asserted of the dense route alone, so a badly placed threshold cannot hide a
failure.  Thresholds are quantiles of the dense values (they depend on the reference only).  Values of common nodes: norm-wise
relative error max|a - b| / max|b| <= 1e-4, the project's base bound (both sides run the same arithmetic).

Run with -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
BAND = 1e-4
DIMS = (13, 11, 9)          # N = 1287: no multiple of 32, more than one selection block (1024) and 11 evaluator workgroups
IMG = 64


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    """kind -> Model with seeded weights (synthetic.py), built once."""
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model
    cache = {}

    def get(kind, adim):
        if (kind, adim) not in cache:
            cfg = model_cfg_from_dict({"action_dim": adim, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                                       "action_decoder": {"name": kind}})
            model = Model(cfg)
            model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes(kind, adim), seed=0), strict=True)
            cache[(kind, adim)] = model.to(dev).eval().requires_grad_(False)
        return cache[(kind, adim)]

    return get


def _grid():
    """In front of the identity context camera (normalised focal 0.8): the near corners project outside the image."""
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), DIMS)   # (no node ON an image border)


def _camera_input(batch, dev, seed=0):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.model import CameraInput
    cams = synthetic.synthetic_cameras(batch)
    c2w = cams["ctxt_c2w"].clone()
    if batch > 1:   # the second image looks from another pose: the batch element of a node must pick ITS camera
        c2w[1:] = synthetic.general_pose(7, batch - 1, scale=0.05)
    # (0.03 x: the seeded trunk maps a [0, 1] image to features of ~100, which overflow exp() in the density heads; this keeps
    #  them at the O(1) scale of synthetic.synthetic_features, for which the seeded decoder weights are made)
    image = 0.03 * torch.rand(batch, 3, IMG, IMG, generator=torch.Generator().manual_seed(11 + seed))
    return CameraInput(input_image=image.to(dev), ctxt_extrinsics=c2w.to(dev), ctxt_intrinsics=cams["ctxt_k_norm"].to(dev),
                       trgt_extrinsics=c2w.to(dev), trgt_intrinsics=cams["ctxt_k_norm"].to(dev))


def _encoding(model, cam, adim, features=None, seed=1):
    """PixelEncoding on the synthetic scene's feature map (synthetic.synthetic_features, N(0, 1)), or on `features`."""
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    b, dev = cam.input_image.shape[0], cam.input_image.device
    feats = synthetic.synthetic_features(b, IMG, IMG, seed=seed).to(dev) if features is None else features
    return PixelEncoding(features=feats, extrinsics=cam.ctxt_extrinsics, intrinsics=cam.ctxt_intrinsics,
                         action=synthetic.synthetic_action(cam.input_image.shape[0], adim).to(cam.input_image.device))


def _dense(model, enc, grid, view_direction=(0.0, 0.0, 1.0), want_jacobian=True):
    """The existing dense route on grid.points(): every per-node field as [B*N, ...]."""
    b = enc.extrinsics.shape[0]
    dev = enc.extrinsics.device
    xyz = grid.points(device=dev)
    n = xyz.shape[0]
    xyzb = xyz[None].expand(b, n, 3).contiguous()
    head, extras = model.compute_density(xyzb, enc)
    out = {"xyz": xyz.repeat(b, 1), "density": head.density.reshape(b * n).clone()}
    if want_jacobian:
        out["jacobian"] = extras["jacobian_head_output"].reshape(b * n, -1, 3).clone()
    dirs = torch.tensor(view_direction, dtype=torch.float32, device=dev).expand(b, n, 1, 3).contiguous()
    out["color"] = model.decoder.forward(xyzb[:, :, None, :].contiguous(), dirs, enc).color.reshape(b * n, 3).clone()
    out["proposal"] = model.proposal_networks[-1].get_density(xyzb[:, :, None, :].contiguous(), enc).reshape(b * n).clone()
    return out


def _quantile_threshold(values, keep_fraction):
    """A threshold that keeps ~keep_fraction of `values`, placed half-way between two neighbouring dense values."""
    s = torch.sort(values.double().cpu()).values
    k = min(max(int(round((1.0 - keep_fraction) * s.numel())), 1), s.numel() - 1)
    return float(0.5 * (s[k - 1] + s[k]))


def _band(values, threshold):
    return (values.double() - threshold).abs() <= BAND * abs(threshold)


def _check_set(index, keep, band, dense_count):
    """`index` (ascending int32 global indices) equals nonzero(keep) up to the nodes of `band`, which are at most 1 % of the
    dense set.  Returns the indices common to both."""
    assert int(band.sum()) <= 0.01 * dense_count, ("threshold badly placed: band too large", int(band.sum()), dense_count)
    idx = index.long()
    assert idx.numel() < 2 or bool((idx[1:] > idx[:-1]).all()), "indices are not strictly ascending"
    got = torch.zeros_like(keep)
    got[idx] = True
    assert int(got.sum()) == idx.numel()
    wrong = (got != keep) & ~band
    assert not bool(wrong.any()), ("set differs outside the band", torch.nonzero(wrong).flatten()[:8].tolist())
    return torch.nonzero(got & keep).flatten()


def _check_rows(cloud, dense, common, grid, exact=False, fields=("density", "color", "jacobian")):
    """Rows of the common nodes against the gathered dense rows; xyz bit-equal to grid.points(index) and to the CPU evaluation."""
    n = cloud.valid()
    index = cloud.index[:n].long()
    assert torch.equal(cloud.xyz[:n], grid.points(cloud.index[:n]))
    assert torch.equal(cloud.xyz[:n].cpu(), grid.points(cloud.index[:n].cpu()))
    assert torch.equal(cloud.xyz[:n], dense["xyz"][index])
    assert torch.equal(cloud.batch_index[:n].long(), index // grid.num_nodes)
    rows = torch.searchsorted(index, common)
    assert torch.equal(index[rows], common)
    report = {}
    for name in fields:
        got, ref = getattr(cloud, name)[:n][rows], dense[name][common]
        report[name] = (rel(got, ref), bool(torch.equal(got, ref)))
        if exact:
            assert torch.equal(got, ref), (name, report[name])
        assert report[name][0] <= TOL, (name, report[name])
    print("field rows (rel, bit-equal):", report)
    return report


# ---- 1. exact mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("precision", ["f32", None, "f16"])
@pytest.mark.parametrize("kind,adim", [("jacobian_mlp", 8), ("jacobian_transformer", 6)])
def test_exact_mode_equals_the_dense_route(models, dev, kind, adim, precision, batch):
    """cull=None, in_frustum=False: by definition the dense route restricted to density >= threshold.  Density, colour and
    Jacobian rows are BIT-EQUAL to the gathered dense rows in all twelve cases, asserted with torch.equal in every precision:
    both routes run the one evaluator body (points_kernel, fed from the grid list here and from the point list there) and a
    point's result does not depend on its tile.  (Observed on the MI355X also while the two routes had a kernel each.)"""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models(kind, adim)
    model.set_precision(hip.DEFAULT_PRECISION if precision is None else precision)
    try:
        grid = _grid()
        enc = _encoding(model, _camera_input(batch, dev), adim)
        dense = _dense(model, enc, grid)
        thr = _quantile_threshold(dense["density"], 0.3)
        keep = dense["density"] >= thr
        cloud = extract_field(model, enc, grid, thr, cull=None, in_frustum=False)
        assert cloud.index.dtype == torch.int32 and tuple(cloud.jacobian.shape) == (cloud.index.shape[0], adim, 3)
        assert int(cloud.count.item()) == cloud.index.shape[0] == cloud.xyz.shape[0] == cloud.density.shape[0]
        assert cloud.stage_names == ("density",)
        common = _check_set(cloud.index, keep, _band(dense["density"], thr), int(keep.sum()))
        assert common.numel() > 0.2 * keep.numel()
        _check_rows(cloud, dense, common, grid, exact=True)
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


# ---- 2. cull --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,adim", [("jacobian_mlp", 8), ("jacobian_transformer", 6)])
def test_cull_equals_the_intersection_of_the_two_dense_sets(models, dev, kind, adim):
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models(kind, adim)
    grid = _grid()
    enc = _encoding(model, _camera_input(2, dev), adim)
    dense = _dense(model, enc, grid)
    thr = _quantile_threshold(dense["density"], 0.5)
    c = _quantile_threshold(dense["proposal"], 0.35)
    passed = dense["proposal"] >= c
    assert int((~passed).sum()) >= 0.5 * passed.numel(), "the cull must remove at least half of the grid"
    keep = passed & (dense["density"] >= thr)
    band = _band(dense["proposal"], c) | _band(dense["density"], thr)
    cloud = extract_field(model, enc, grid, thr, cull=c, in_frustum=False)
    assert cloud.stage_names == ("proposal", "density")
    after_cull = int(cloud.stage_counts[0].item())
    assert abs(after_cull - int(passed.sum())) <= int(_band(dense["proposal"], c).sum())
    common = _check_set(cloud.index, keep, band, int(keep.sum()))
    assert common.numel() > 0
    _check_rows(cloud, dense, common, grid)
    # the last proposal network is the default level
    again = extract_field(model, enc, grid, thr, cull=c, in_frustum=False, proposal_level=len(model.proposal_networks) - 1)
    assert torch.equal(again.index, cloud.index)


# ---- 3. frustum -----------------------------------------------------------------------------------------------------------
def _projection_predicate(enc, xyz_all, nodes):
    """float64 torch evaluation of the gather's projection: (inside, band) per global node; band = within 16 fp32 ulps of 1
    (the normalised image coordinate's scale) of an image border, or of zero depth."""
    b = enc.extrinsics.shape[0]
    w2c = torch.linalg.inv(enc.extrinsics.double())
    p = xyz_all.double().reshape(b, nodes, 3)
    cam = torch.einsum("bij,bnj->bni", w2c[:, :3, :3], p) + w2c[:, None, :3, 3]
    uvw = torch.einsum("bij,bnj->bni", enc.intrinsics.double(), cam)
    u, v, z = uvw[..., 0] / (uvw[..., 2] + 1e-9), uvw[..., 1] / (uvw[..., 2] + 1e-9), cam[..., 2]
    inside = (z > 0) & (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
    eps = 16 * 2.0 ** -23
    band = (u.abs() <= eps) | ((u - 1).abs() <= eps) | (v.abs() <= eps) | ((v - 1).abs() <= eps) | (z.abs() <= eps)
    return inside.reshape(-1), band.reshape(-1)


def test_frustum_equals_the_dense_set_inside_the_context_view(models, dev):
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models("jacobian_mlp", 8)
    grid = _grid()
    enc = _encoding(model, _camera_input(2, dev), 8)
    dense = _dense(model, enc, grid)
    inside, border = _projection_predicate(enc, dense["xyz"], grid.num_nodes)
    assert 0.1 * inside.numel() < int(inside.sum()) < 0.9 * inside.numel(), "the grid must lie partly outside the view"
    assert bool(inside.reshape(2, -1)[0].ne(inside.reshape(2, -1)[1]).any()), "the two cameras must see different node sets"
    thr = _quantile_threshold(dense["density"], 0.5)
    keep = inside & (dense["density"] >= thr)
    cloud = extract_field(model, enc, grid, thr, in_frustum=True)
    assert cloud.stage_names == ("frustum", "density")
    assert abs(int(cloud.stage_counts[0].item()) - int(inside.sum())) <= int(border.sum())
    common = _check_set(cloud.index, keep, border | _band(dense["density"], thr), int(keep.sum()))
    _check_rows(cloud, dense, common, grid)
    # all three predicates together
    c = _quantile_threshold(dense["proposal"], 0.5)
    keep3 = keep & (dense["proposal"] >= c)
    cloud3 = extract_field(model, enc, grid, thr, cull=c, in_frustum=True)
    assert cloud3.stage_names == ("frustum", "proposal", "density")
    common3 = _check_set(cloud3.index, keep3, border | _band(dense["density"], thr) | _band(dense["proposal"], c), int(keep3.sum()))
    _check_rows(cloud3, dense, common3, grid)


def test_view_direction_reaches_the_colour_head(models, dev):
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models("jacobian_mlp", 8)
    grid = _grid()
    enc = _encoding(model, _camera_input(1, dev), 8)
    direction = (0.6, -0.48, 0.64)
    dense = _dense(model, enc, grid, view_direction=direction)
    thr = _quantile_threshold(dense["density"], 0.3)
    cloud = extract_field(model, enc, grid, thr, in_frustum=False, view_direction=direction)
    common = _check_set(cloud.index, dense["density"] >= thr, _band(dense["density"], thr), int((dense["density"] >= thr).sum()))
    _check_rows(cloud, dense, common, grid)
    default = extract_field(model, enc, grid, thr, in_frustum=False)
    assert torch.equal(default.index, cloud.index) and not torch.equal(default.color, cloud.color)


# ---- 4. determinism -------------------------------------------------------------------------------------------------------
def _fields(cloud):
    n = cloud.valid()
    out = {"count": cloud.count, "index": cloud.index[:n], "xyz": cloud.xyz[:n], "density": cloud.density[:n]}
    if cloud.color is not None:
        out["color"] = cloud.color[:n]
    if cloud.jacobian is not None:
        out["jacobian"] = cloud.jacobian[:n]
    out.update({f"stage_{i}": c for i, c in enumerate(cloud.stage_counts)})
    return out


def _assert_same(a, b):
    fa, fb = _fields(a), _fields(b)
    assert fa.keys() == fb.keys()
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k


@pytest.fixture(scope="module")
def full_case(models, dev):
    """One scene with all three predicates enabled and its unconstrained (eager) result, shared by the tests below."""
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models("jacobian_mlp", 8)
    grid = _grid()
    enc = _encoding(model, _camera_input(2, dev), 8)
    dense = _dense(model, enc, grid)
    kw = dict(density_threshold=_quantile_threshold(dense["density"], 0.6), cull=_quantile_threshold(dense["proposal"], 0.6),
              in_frustum=True)
    cloud = extract_field(model, enc, grid, **kw)
    assert cloud.index.shape[0] > 64
    return model, grid, enc, kw, cloud


def test_two_calls_give_equal_bytes(full_case):
    from neural_jacobian_field_amd.field_volume import extract_field
    model, grid, enc, kw, cloud = full_case
    _assert_same(cloud, extract_field(model, enc, grid, **kw))
    padded = extract_field(model, enc, grid, max_points=cloud.index.shape[0] + 37, **kw)
    _assert_same(padded, extract_field(model, enc, grid, max_points=cloud.index.shape[0] + 37, **kw))


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------
def test_capacity_keeps_the_first_rows_and_the_true_count(full_case):
    from neural_jacobian_field_amd.field_volume import extract_field
    model, grid, enc, kw, cloud = full_case
    true = cloud.index.shape[0]
    for m in (true - 33, 1, true, true + 50):
        got = extract_field(model, enc, grid, max_points=m, **kw)
        assert got.index.shape[0] == m and got.jacobian.shape[0] == m
        assert int(got.count.item()) == true                       # the TRUE count, also when it exceeds the capacity
        assert [int(c.item()) for c in got.stage_counts] == [int(c.item()) for c in cloud.stage_counts]
        k = min(m, true)
        assert got.valid() == k
        for name in ("index", "xyz", "density", "color", "jacobian"):
            assert torch.equal(getattr(got, name)[:k], getattr(cloud, name)[:k]), (m, name)


# ---- 6. capture -----------------------------------------------------------------------------------------------------------
def test_capture_on_static_features_replays_a_second_image_exactly(full_case, dev):
    """The max_points form has no host synchronisation: it is captured (one stream) and replayed after the feature map of a
    second image was copied into the captured input; everything equals the eager result on those features bit for bit."""
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import extract_field
    model, grid, enc, kw, cloud = full_case
    m = cloud.index.shape[0] + 200
    from neural_jacobian_field_amd import synthetic
    feats2 = synthetic.synthetic_features(2, IMG, IMG, seed=9).to(dev)
    static = PixelEncoding(features=enc.features.clone(), extrinsics=enc.extrinsics, intrinsics=enc.intrinsics, action=None)
    extract_field(model, static, grid, max_points=m, **kw)      # eager warm-up: packed weights, device constants
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = extract_field(model, static, grid, max_points=m, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _assert_same(captured, cloud)                                # first image
    static.features.copy_(feats2)
    graph.replay()
    torch.cuda.synchronize()
    enc2 = PixelEncoding(features=feats2, extrinsics=enc.extrinsics, intrinsics=enc.intrinsics, action=None)
    eager2 = extract_field(model, enc2, grid, **kw)
    assert not torch.equal(eager2.index, cloud.index), "the second image must give another cloud"
    assert eager2.index.shape[0] <= m
    _assert_same(captured, eager2)


def test_model_extract_field_captures_with_the_encoder_inside(models, dev):
    """Model.extract_field(max_points=M) -- image encoder included -- captured and replayed with a second image, against the
    dense route on that image's features (the encoder's convolutions are not bit-reproducible from run to run, so the
    comparison is the band rule + 1e-4 as everywhere, not bit equality)."""
    from neural_jacobian_field_amd.model import CameraInput
    model = models("jacobian_mlp", 8)
    grid = _grid()
    cam1, cam2 = _camera_input(1, dev, seed=1), _camera_input(1, dev, seed=2)
    with torch.no_grad():
        enc2 = _encoding(model, cam2, 8, features=model._encode_for_render(cam2.input_image))
    dense = _dense(model, enc2, grid)
    thr, c = _quantile_threshold(dense["density"], 0.6), _quantile_threshold(dense["proposal"], 0.6)
    inside, border = _projection_predicate(enc2, dense["xyz"], grid.num_nodes)
    keep = inside & (dense["proposal"] >= c) & (dense["density"] >= thr)
    band = border | _band(dense["proposal"], c) | _band(dense["density"], thr)
    m = int(keep.sum()) + 200
    static = CameraInput(input_image=cam1.input_image.clone(), ctxt_extrinsics=cam1.ctxt_extrinsics,
                         ctxt_intrinsics=cam1.ctxt_intrinsics, trgt_extrinsics=cam1.trgt_extrinsics,
                         trgt_intrinsics=cam1.trgt_intrinsics)
    for _ in range(2):                                           # eager warm-up (library solver searches, constants)
        model.extract_field(static, grid, thr, cull=c, max_points=m)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = model.extract_field(static, grid, thr, cull=c, max_points=m)
    static.input_image.copy_(cam2.input_image)
    graph.replay()
    torch.cuda.synchronize()
    n = captured.valid()
    assert n == int(captured.count.item())
    common = _check_set(captured.index[:n], keep, band, int(keep.sum()))
    assert common.numel() > 0
    _check_rows(captured, dense, common, grid)
    eager = model.extract_field(cam2, grid, thr, cull=c)         # the exactly sized form of the same call
    assert abs(eager.index.shape[0] - n) <= int(band.sum())


# ---- 7. refusals and colouring ----------------------------------------------------------------------------------------------
def test_flow_mlp_refuses_a_jacobian_and_works_without(models, dev):
    from neural_jacobian_field_amd.field_volume import extract_field
    model = models("flow_mlp", 5)
    grid = _grid()
    cam = _camera_input(1, dev)
    with pytest.raises(NotImplementedError, match="no Jacobian"):
        model.extract_field(cam, grid, 0.3)
    enc = _encoding(model, cam, 5)
    dense = _dense(model, enc, grid, want_jacobian=False)
    thr = _quantile_threshold(dense["density"], 0.4)
    keep = dense["density"] >= thr
    cloud = extract_field(model, enc, grid, thr, in_frustum=False, want_jacobian=False)
    assert cloud.jacobian is None and cloud.color is not None
    common = _check_set(cloud.index, keep, _band(dense["density"], thr), int(keep.sum()))
    _check_rows(cloud, dense, common, grid, fields=("density", "color"))
    bare = extract_field(model, enc, grid, thr, in_frustum=False, want_jacobian=False, want_color=False)
    assert bare.color is None and torch.equal(bare.index, cloud.index) and torch.equal(bare.density, cloud.density)
    via_model = model.extract_field(cam, grid, thr, want_jacobian=False)      # image encoder included
    assert via_model.jacobian is None and via_model.index.shape[0] == int(via_model.count.item())


def test_cloud_colours_and_ply(full_case, tmp_path):
    model, grid, enc, kw, cloud = full_case
    colors = cloud.colors("model_allegro")
    assert tuple(colors.shape) == (cloud.index.shape[0], 3) and colors.device == cloud.jacobian.device
    assert float(colors.min()) >= 0.0 and float(colors.max()) <= 1.0
    assert cloud.save_ply(tmp_path / "field.ply", colors=colors) == cloud.index.shape[0]
    raw = open(tmp_path / "field.ply", "rb").read()
    payload = raw[raw.index(b"end_header\n") + 11:]
    assert len(payload) == cloud.index.shape[0] * 19
    first = np.frombuffer(payload[:12], dtype="<f4")
    assert np.array_equal(first, cloud.xyz[0].cpu().numpy())


def test_nothing_survives_an_unreachable_threshold(full_case):
    from neural_jacobian_field_amd.field_volume import extract_field
    model, grid, enc, kw, cloud = full_case
    empty = extract_field(model, enc, grid, 1e30, in_frustum=False)
    assert empty.index.shape[0] == 0 and int(empty.count.item()) == 0 and tuple(empty.jacobian.shape) == (0, 8, 3)
    padded = extract_field(model, enc, grid, 1e30, in_frustum=False, max_points=16)
    assert int(padded.count.item()) == 0 and padded.valid() == 0 and padded.index.shape[0] == 16
