"""GPU tests of the back-projection of depth frames (field_volume.depth_points; njf_field_depth_points).

The points are held to the torch expression ``origins + directions * t`` formed from ``geometry.full_frame_rays`` BYTE FOR BYTE
-- the kernel restates the ray kernel's arithmetic and adds one multiply and one add --, the validity rules to the numpy
restatement's mask (tests/field_voxels_restatement.py) bit for bit, and the points once more to a float64 pinhole model
within the fp32 rounding of the chain (1e-5 of the scene's scale).

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_voxels_restatement as S

pytestmark = pytest.mark.gpu

FRAMES = ((1, 1), (1, 65), (5, 7), (3, 257))       # one pixel, a row crossing a wave, an odd frame, a row crossing a workgroup


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _cameras(batch, seed):
    """Rotated and translated cameras; the first has a non-square intrinsic, the others differ from it."""
    rng = np.random.default_rng(seed)
    k, c2w = np.zeros((batch, 3, 3), np.float32), np.zeros((batch, 4, 4), np.float32)
    for i in range(batch):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q *= np.sign(np.linalg.det(q))
        c2w[i, :3, :3], c2w[i, :3, 3], c2w[i, 3, 3] = q, rng.uniform(-2, 2, 3), 1.0
        fx, fy = (0.8, 1.1) if i == 0 else rng.uniform(0.6, 1.4, 2)
        k[i] = [[fx, 0.0, 0.5 + 0.02 * i], [0.0, fy, 0.5 - 0.01 * i], [0.0, 0.0, 1.0]]
    return k, c2w


def _depth(batch, h, w, seed, dirty=True):
    """Depths of 1 to 3 in smooth patches with steps between them; with ``dirty`` a sprinkling of 0, NaN, inf and negatives."""
    rng = np.random.default_rng(seed)
    d = (1.0 + rng.integers(0, 3, (batch, h, w)) * 0.7 + rng.uniform(0, 0.05, (batch, h, w))).astype(np.float32)
    if dirty and h * w > 4:
        flat = d.reshape(batch, -1)
        for i in range(batch):
            bad = rng.permutation(h * w)[:max(4, h * w // 6)]
            flat[i, bad] = np.resize(np.float32([0.0, np.nan, np.inf, -1.5, -np.inf, -0.0]), bad.shape[0])
    return d


def _want(dev, depth, k, c2w, kind):
    """origins + directions * t from full_frame_rays, in torch on the device."""
    from neural_jacobian_field_amd.geometry import full_frame_rays
    b, h, w = depth.shape
    origins, directions, z = full_frame_rays(h, w, k, c2w)
    t = depth.reshape(b, h * w, 1)
    if kind == "z":
        t = t / z
    return origins + directions * t


def _check(dev, depth, k, c2w, kind, views=1, **rules):
    from neural_jacobian_field_amd.field_volume import depth_points
    d, kk, cc = (torch.from_numpy(v).to(dev) for v in (depth, k, c2w))
    got = depth_points(d, kk, cc, kind=kind, views_per_scene=views, **rules)
    b, h, w = depth.shape
    assert got.points.shape == (b // views, views * h * w, 3) and got.points.dtype == torch.float32
    assert got.kept.shape == (b // views,) and got.kept.dtype == torch.int32
    mask = S.depth_mask(depth, **rules)
    want = _np(_want(dev, d, kk, cc, kind)).reshape(b, h * w, 3)
    points = _np(got.points).reshape(b, h * w, 3)
    flat = mask.reshape(b, h * w)
    assert np.isnan(points[~flat]).all()                                            # three NaNs where there is no point
    assert points[flat].tobytes() == want[flat].tobytes()                           # the torch expression, byte for byte
    assert _np(got.kept).tolist() == mask.reshape(b // views, -1).sum(axis=1).tolist()
    # ... and a pinhole model in float64: the fp32 chain (inverse, ray, normalisation, t, point) rounds a few times
    ref = S.pinhole_points(depth, k, c2w, kind)
    if flat.any():
        scale = np.abs(ref[flat]).max()
        assert np.abs(points[flat].astype(np.float64) - ref[flat]).max() <= 1e-5 * scale
    return got, mask


@pytest.mark.parametrize("kind", ["ray", "z"])
@pytest.mark.parametrize("batch", [1, 3])
def test_points_equal_the_torch_expression_byte_for_byte(dev, kind, batch):
    for h, w in FRAMES:
        k, c2w = _cameras(batch, seed=h * w + batch)
        _, mask = _check(dev, _depth(batch, h, w, seed=w), k, c2w, kind)
        assert mask.any()
        clean, mask = _check(dev, _depth(batch, h, w, seed=w + 1, dirty=False), k, c2w, kind)
        assert mask.all() and torch.isfinite(clean.points).all()


@pytest.mark.parametrize("rules", [dict(near=1.2), dict(far=2.0), dict(near=1.02, far=2.43), dict(max_jump=0.1), dict(max_jump=0.5),
                                   dict(max_jump=1e-3), dict(near=1.02, far=2.43, max_jump=0.3)])
def test_validity_rules_equal_the_restatement_bit_for_bit(dev, rules):
    for h, w in ((5, 7), (3, 257), (1, 65)):
        k, c2w = _cameras(3, seed=7)
        depth = _depth(3, h, w, seed=h + w)
        depth[0, 0, 0], depth[1, -1, -1] = np.float32(rules.get("near", 1.0)), np.float32(rules.get("far", 2.0))   # on the limits themselves
        _, mask = _check(dev, depth, k, c2w, "z", **rules)
        plain = S.depth_mask(depth)
        assert 0 < mask.sum() < plain.sum() or (rules == dict(max_jump=1e-3) and mask.sum() < plain.sum())
        if "near" in rules:
            assert not mask[0, 0, 0]                                                # near < d is strict
        if "far" in rules and "max_jump" not in rules:
            assert mask[1, -1, -1]                                                  # d <= far is not


def test_the_hand_written_edge_image(dev):
    nan = np.nan
    depth = np.float32([[[1.00, 1.04, 2.00, 2.05], [1.00, 0.00, 2.00, nan], [1.02, 1.05, 1.09, 2.10]]])
    k, c2w = _cameras(1, seed=3)
    got, mask = _check(dev, depth, k, c2w, "ray", max_jump=0.1)
    assert mask[0].tolist() == [[True, False, False, True], [True, False, False, False], [True, True, False, False]]
    assert int(got.kept[0]) == 5


def test_the_views_of_a_scene_are_one_cloud(dev):
    from neural_jacobian_field_amd.field_volume import depth_points
    k, c2w = _cameras(4, seed=11)
    depth = _depth(4, 5, 7, seed=2)
    depth[2] = 0.0                                                                  # a view that saw nothing
    two, mask = _check(dev, depth, k, c2w, "z", views=2, max_jump=0.5)
    one = depth_points(*(torch.from_numpy(v).to(dev) for v in (depth, k, c2w)), max_jump=0.5)
    assert two.points.shape == (2, 70, 3) and one.points.shape == (4, 35, 3)
    assert torch.equal(_bytes(two.points), _bytes(one.points.reshape(2, 70, 3)))
    assert torch.equal(two.kept, one.kept.reshape(2, 2).sum(dim=1).to(torch.int32)) and int(one.kept[2]) == 0
    four, _ = _check(dev, depth, k, c2w, "z", views=4, max_jump=0.5)
    assert four.points.shape == (1, 140, 3) and int(four.kept[0]) == int(mask.sum())


def test_every_row_is_written_and_calls_and_a_captured_replay_agree(dev):
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import depth_points
    k, c2w = _cameras(3, seed=5)
    depth = _depth(3, 3, 257, seed=9)
    d, kk, cc = (torch.from_numpy(v).to(dev) for v in (depth, k, c2w))
    kw = dict(kind="z", near=1.01, far=2.44, max_jump=0.25)
    first, second = (depth_points(d, kk, cc, **kw) for _ in range(2))
    assert torch.equal(_bytes(first.points), _bytes(second.points)) and torch.equal(first.kept, second.kept)
    for fill in (0x00, 0xa5):                                                       # 0xa5a5a5a5 is a finite float and a large count
        points = torch.empty(3, 3 * 257, 3, device=dev)
        kept = torch.empty(3, dtype=torch.int32, device=dev)
        for t in (points, kept):
            t.view(torch.uint8).fill_(fill)
        hip.field_depth_points(d, hip.inverse(kk).contiguous(), cc, hip.FIELD_DEPTH_Z, float(np.float32(1.01)), float(np.float32(2.44)),
                               0.25, 1, points, kept)
        assert torch.equal(_bytes(points), _bytes(first.points)) and torch.equal(kept, first.kept), fill
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = depth_points(d, kk, cc, **kw)
    for t in (out.points, out.kept):
        t.view(torch.uint8).fill_(0x77)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bytes(out.points), _bytes(first.points)) and torch.equal(out.kept, first.kept)
    assert 0 < int(first.kept.sum()) < 3 * 3 * 257
