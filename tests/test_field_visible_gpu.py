"""GPU tests of the z-buffer of posed rows (field_volume.visible_rows / FieldView / register_commands_visible;
njf_field_visible) against the numpy restatement of its semantics (tests/field_visible_restatement.py), in two layers, so that exactness
is asked only where it can hold.

Layer 1, the projection: the device's ``z`` within 1e-5 of the float64 pinhole model -- the bound ``depth_points`` is held to --
and its ``pixel`` EQUAL to the model's on every row.  The clouds are built by back-projecting chosen pixel positions, and the
test first asserts, with the restatement, that no row lies within 1e-3 pixels of a pixel edge or within 1e-4 of ``near``: an
fp32 projection at these sizes is off by 1e-4 pixels at the most.

Layer 2, everything else, from the device's OWN ``pixel`` and ``z``: depth, index, covered, seen, visible and culled equal
``rasterise`` and ``test_rows`` byte for byte, in both forms of the splat, on sentinel-filled outputs.

End to end (test_the_whole_shell_registers_to_a_depth_image): the scene of section 22 with ALL 878 shell rows.  Measured on an
MI355X: |u - planted| = 3.945e-2 with the cull (restatement 3.945e-2, 175 rows visible in every round, equal to the
restatement's counts) and 7.195e-1 without.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_joints_restatement as J
import field_nearest_restatement as N
import field_visible_restatement as V
import field_voxels_restatement as S
from test_field_commands_gpu import Scene
from test_field_nearest_gpu import _register, _scene_cells
from test_field_normals_gpu import _shell
from test_field_voxels_gpu import ANGLES, CONVERGED, HEIGHT, MAX_JUMP, ROUNDS, SHELL_MODEL, SHELL_SEEN, WIDTH, _camera, _z_buffer

pytestmark = pytest.mark.gpu

F32 = np.float32
OUT = ("depth", "index", "covered", "seen", "culled", "visible", "pixel", "z")
ROWS = (1, 63, 64, 65, 257, 4097)
IMAGES = ((1, 1), (1, 7), (5, 3), (48, 64))
PROBLEMS = ((1, 1, 1), (3, 3, 1), (3, 3, 3), (1, 3, 3))            # (V, M, Mq)
EDGE, NEAR_MARGIN, Z_BOUND = 1e-3, 1e-4, 1e-5


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


def _cameras(views):
    """``views`` cameras around section 22's: the same intrinsics, the pose turned and shifted a little per view."""
    k, c2w = _camera()
    ks, poses = [], []
    for v in range(views):
        a = 0.07 * v
        turn = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
        pose = c2w[0].astype(np.float64) @ turn
        pose[:3, 3] += (0.05 * v, -0.03 * v, 0.02 * v)
        ks.append(k[0] * np.array([[1 + 0.1 * v], [1 - 0.05 * v], [1]]))
        poses.append(pose)
    return np.stack(ks).astype(F32), np.stack(poses).astype(F32)


def _margins(pr, near):
    """The distance of every projectable row to the nearest pixel edge, in pixels, and of every finite z to ``near``."""
    edge = np.minimum(np.abs(pr["x"] - np.rint(pr["x"])), np.abs(pr["y"] - np.rint(pr["y"])))
    edge = np.where(pr["projectable"] & np.isfinite(edge), edge, np.inf)
    return edge, np.where(np.isfinite(pr["z"]), np.abs(pr["z"] - float(F32(near))), np.inf)


def _cloud(rng, k, c2w, sets, n, height, width, near=0.0, reach=2.6, dirty=True):
    """[sets, n, 3] fp32: pixel positions in and around the image of camera 0, back-projected at a depth in [1, 3] -- a tenth of
    the rows behind the camera --, redrawn until no row lies near a pixel edge or near ``near`` in any view.  With ``dirty`` three
    rows are not finite."""
    k64, c64 = np.asarray(k, np.float64), np.asarray(c2w, np.float64)

    def draw(count):
        x = rng.uniform(-reach, width + reach, count)
        y = rng.uniform(-reach, height + reach, count)
        z = rng.uniform(1.0, 3.0, count) * np.where(rng.random(count) < 0.1, -1.0, 1.0)
        z = np.where(rng.random(count) < 0.3, np.round(z * 4) / 4, z)              # a few shared depths
        cam = np.stack([x / width, y / height, np.ones(count)], axis=1) @ np.linalg.inv(k64[0]).T * z[:, None]
        return (cam @ c64[0, :3, :3].T + c64[0, :3, 3]).astype(F32)

    pts = draw(sets * n).reshape(sets, n, 3)
    pts[:, 0] = draw(sets * 8).reshape(sets, 8, 3)[:, 0]                            # (any row may be anywhere)
    for _ in range(200):
        edge, to_near = _margins(V.project(pts, k, c2w, height, width, near), near)
        bad = ((edge < 2 * EDGE) | (to_near < 2 * NEAR_MARGIN)).any(axis=1)
        if not bad.any():
            break
        pts[bad] = draw(int(bad.sum()))
    assert not bad.any()
    if dirty and n >= 8:
        pts[:, 3, 1], pts[:, n // 2, 0], pts[:, -2] = np.nan, np.inf, -np.inf
    return pts


def _outputs(dev, m, views, n, height, width, fill=None):
    from neural_jacobian_field_amd import hip
    shapes = dict(depth=(m, views, height, width), index=(m, views, height, width), covered=(m, views), seen=(m, n), culled=(m, n, 3),
                  visible=(m,), pixel=(m, views, n), z=(m, views, n))
    out = {f: torch.empty(shapes[f], dtype=dtype, device=dev) for f, dtype in hip.FIELD_VISIBLE_OUTPUTS}
    if fill is not None:
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
    return out


def _raw(dev, points, k, c2w, height, width, m, phase, fill=None, out=None, workspace=None, w2c=None, **kw):
    """hip.field_visible on outputs of the test's own, optionally sentinel-filled; a dict of tensors."""
    from neural_jacobian_field_amd import hip
    w2c = hip.inverse(_t(dev, c2w)) if w2c is None else _t(dev, w2c)
    out = _outputs(dev, m, k.shape[0], points.shape[1], height, width, fill) if out is None else out
    hip.field_visible(points, _t(dev, k), w2c, height, width, out, m, phase=phase, workspace=workspace, **kw)
    return out


def _layer_1(got, pts, k, c2w, height, width, near, count, labels, what):
    """The device's pixel and z against the float64 model, on every row; returns the model and the read rows."""
    pr = V.project(pts, k, c2w, height, width, near)
    edge, to_near = _margins(pr, near)
    read = V.read_rows(pts, count, labels)
    assert edge[np.broadcast_to(read[:, None], edge.shape)].min(initial=np.inf) >= EDGE, what
    assert to_near[np.broadcast_to(read[:, None], edge.shape)].min(initial=np.inf) >= NEAR_MARGIN, what
    m = got["pixel"].shape[0]
    worst = 0.0
    for i in range(m):
        q = 0 if pts.shape[0] == 1 else i
        rows = np.broadcast_to(read[q][None], pr["pixel"][q].shape)
        assert (got["pixel"][i] == np.where(rows, pr["pixel"][q], -1)).all(), (what, "pixel")
        assert np.isnan(got["z"][i][~rows]).all(), (what, "z of rows that are not read")
        dz = np.abs(got["z"][i][rows].astype(np.float64) - pr["z"][q][rows])
        worst = max(worst, float(dz.max(initial=0.0)))
    assert worst <= Z_BOUND, (what, worst)
    return pr, read, worst


def _layer_2(got, pts, pr, read, m, height, width, footprint, tolerance, what):
    """Every output against the restatement from the device's own pixel and z: equal bytes."""
    mq = pts.shape[0]
    want = V.finish(pts, got["pixel"][:mq].astype(np.int64), got["z"][:mq], read,
                    lambda q, v: V.outside_rows(pr, q, v, footprint, height, width), m, height, width, footprint, tolerance)
    for f in OUT:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].dtype, got[f].shape)
        differ = int((got[f].view(np.uint8) != want[f].view(np.uint8)).sum())
        assert differ == 0, (what, f, differ)
    return want


def _check(dev, pts, k, c2w, height, width, m, footprint, tolerance, near=0.0, count=None, labels=None, what=""):
    """Both forms of the splat on sentinel-filled outputs, through both layers; the public function where it takes the case."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldView, visible_rows
    p, c, l = _t(dev, pts), (None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)), _t(dev, labels)
    kw = dict(count=c, labels=l, footprint=footprint, near=near, tolerance=tolerance)
    want = None
    for phase, fill in ((hip.FIELD_VISIBLE_ALL, 0x5a), (hip.FIELD_VISIBLE_ALL | hip.FIELD_VISIBLE_DIRECT, 0xa5)):
        got = {f: _np(t) for f, t in _raw(dev, p, k, c2w, height, width, m, phase, fill=fill, **kw).items()}
        pr, read, worst = _layer_1(got, pts, k, c2w, height, width, near, count, labels, what)
        want = _layer_2(got, pts, pr, read, m, height, width, footprint, tolerance, f"{what}, phase {phase}")
    if pts.shape[0] == m:
        view = FieldView(_t(dev, k), _t(dev, c2w), height, width, footprint=footprint, tolerance=tolerance, near=near)
        public = visible_rows(p if m > 1 else p[0], view, labels=l, count=c)
        for f in OUT:
            assert _np(getattr(public, f)).tobytes() == want[f].tobytes(), (what, f, "visible_rows")
    return want, worst


# ---- 1. the two layers over the shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,width", IMAGES)
def test_every_output_equals_the_restatement(dev, height, width):
    rng = np.random.default_rng(100 * height + width)
    case, worst, seen_rows, footprints = 0, 0.0, 0, set()
    for n in ROWS:
        for views, m, mq in PROBLEMS:
            footprint = case % 5                                                   # 0 .. 4: larger than the small images
            case += 1
            k, c2w = _cameras(views)
            pts = _cloud(rng, k, c2w, mq, n, height, width)
            count = None if case % 3 else max(n - 3, 0)
            labels = None if case % 4 or n < 8 else np.where(rng.random(n) < 0.1, -1, rng.integers(0, 3, n)).astype(np.int32)
            want, w = _check(dev, pts, k, c2w, height, width, m, footprint, 0.05, count=count, labels=labels,
                             what=f"{height} x {width}, n {n}, V {views}, M {m}, Mq {mq}, f {footprint}")
            worst, seen_rows = max(worst, w), seen_rows + int(want["visible"].sum())
            footprints.add(footprint)
            # properties: a winner of its own pixel is seen in that view; nothing lies in front of the depth
            for i in range(m):
                for v in range(views):
                    flat, pix = want["index"][i, v].reshape(-1), want["pixel"][i, v]
                    own = np.flatnonzero((flat >= 0) & (pix[flat.clip(0)] == np.arange(height * width)))
                    assert ((want["seen"][i][flat[own]] >> v) & 1).all()
                    has = pix >= 0
                    assert (want["depth"][i, v].reshape(-1)[pix[has]] <= want["z"][i, v][has]).all()
    print(f"{height} x {width}: {case} cases, |z - float64| <= {worst:.2e}, {seen_rows} visible rows in all")
    assert footprints == {0, 1, 2, 3, 4} and seen_rows > 0


# ---- 2. further cases -----------------------------------------------------------------------------------------------------------------------
def test_4097_rows_in_one_pixel_with_ties(dev):
    rng = np.random.default_rng(5)
    k, c2w = _cameras(1)
    height, width, n = 5, 3, 4097
    k64, c64 = k.astype(np.float64), c2w.astype(np.float64)
    z = rng.choice([1.25, 1.5, 2.0, 2.75], n)
    xy = np.stack([rng.choice([1.3, 1.5, 1.7], n) / width, rng.choice([2.4, 2.6], n) / height, np.ones(n)], axis=1)
    pts = ((xy @ np.linalg.inv(k64[0]).T * z[:, None]) @ c64[0, :3, :3].T + c64[0, :3, 3]).astype(F32)[None]
    assert np.unique(pts[0], axis=0).shape[0] <= 24                                  # groups of identical points: they tie
    for footprint in (0, 2):
        want, _ = _check(dev, pts, k, c2w, height, width, 1, footprint, 0.0, what=f"one pixel, f {footprint}")
        assert (want["pixel"] == 2 * width + 1).all() and want["covered"][0, 0] == (1 if footprint == 0 else 15)
        zmin = want["z"][0, 0].min()
        first = int(np.flatnonzero(want["z"][0, 0] == zmin)[0])
        assert want["index"][0, 0, 2, 1] == first and want["depth"][0, 0, 2, 1] == zmin          # ties to the lowest row
        assert want["visible"][0] == int((want["z"][0, 0] == zmin).sum()) > 100                 # tolerance 0: the winner's ties


def test_rows_that_are_not_read_behind_the_camera_at_near_and_off_the_image(dev):
    """An identity camera and coordinates that are exact in fp32: the restatement from the float64 model holds byte for byte."""
    from neural_jacobian_field_amd import hip
    k = F32([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]])
    w2c = np.eye(4, dtype=F32)[None]
    near = 0.25
    pts = F32([[-0.375, -0.375, 1.0],      # 0: pixel (0, 0)
               [-0.375, -0.375, 2.0],      # 1: behind row 0 at z 2 (x / z = -0.1875: col 1, row 1)
               [0.0, 0.0, -1.0],           # 2: behind the camera
               [0.0, 0.0, 0.25],           # 3: z == near: not projectable
               [np.nan, 0.0, 1.0],         # 4: not finite
               [0.625, 0.125, 1.0],        # 5: col 4 of 4 -- just off the right edge --, row 2: reaches (1..3, 3) with f = 1
               [0.125, 0.125, 0.5],        # 6: label -1
               [0.3125, 0.125, 1.5],       # 7: pixel (2, 2), z 1.5
               [0.125, 0.125, 1.0],        # 8: from the count on
               [0.125, 0.125, 0.75]])[None]
    labels = np.int32([0, 0, 0, 0, 0, 0, -1, 2, 0, 0])
    p = _t(dev, pts)
    kw = dict(count=torch.tensor([8], dtype=torch.int32, device=dev), labels=_t(dev, labels), near=near, tolerance=0.0)
    for footprint in (0, 1):
        want = V.visible(pts, k, w2c, 4, 4, footprint, 0.0, near, count=8, labels=labels)
        for phase in (hip.FIELD_VISIBLE_ALL, hip.FIELD_VISIBLE_ALL | hip.FIELD_VISIBLE_DIRECT):
            got = _raw(dev, p, k, None, 4, 4, 1, phase, fill=0x5a, w2c=w2c, footprint=footprint, **kw)
            for f in OUT:
                assert _np(got[f]).tobytes() == want[f].tobytes(), (f, footprint, phase)
        assert want["pixel"][0, 0].tolist() == [0, 5, -1, -1, -1, -1, -1, 10, -1, -1]
        assert want["z"][0, 0, :4].tolist() == [1.0, 2.0, -1.0, 0.25] and np.isnan(want["z"][0, 0, [4, 6, 8, 9]]).all()
        assert want["z"][0, 0, 5] == 1.0                                            # read and projectable, with no pixel of its own
    # f = 1: row 5 has no pixel of its own and is not seen, yet it fills (1..3, 3) in front of row 7; row 0's footprint at (1, 1)
    # hides row 1 (z 2 against 1), which still wins the three pixels that only it reaches
    assert want["index"][0, 0].tolist() == [[0, 0, 1, -1], [0, 0, 7, 5], [1, 7, 7, 5], [-1, 7, 7, 5]]
    assert want["seen"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0, 0] and want["covered"].tolist() == [[14]]
    assert V.visible(pts, k, w2c, 4, 4, 0, 0.0, near, count=8, labels=labels)["seen"][0].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 0, 0]


def test_the_phases_one_by_one(dev):
    from neural_jacobian_field_amd import hip
    rng = np.random.default_rng(7)
    k, c2w = _cameras(3)
    height, width, m, n = 5, 3, 3, 257
    pts = _cloud(rng, k, c2w, m, n, height, width)
    p = _t(dev, pts)
    full = _raw(dev, p, k, c2w, height, width, m, hip.FIELD_VISIBLE_ALL, fill=0x11, footprint=1)
    for form in (0, hip.FIELD_VISIBLE_DIRECT):
        workspace = torch.full((hip.field_visible_workspace(m, 3, height, width),), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        out = _outputs(dev, m, 3, n, height, width, fill=0x5a)
        _raw(dev, p, k, c2w, height, width, m, hip.FIELD_VISIBLE_SPLAT | form, out=out, workspace=workspace, footprint=1)
        assert all((_np(t).view(np.uint8) == 0x5a).all() for t in out.values())     # the splat writes the workspace only
        _raw(dev, p, k, c2w, height, width, m, hip.FIELD_VISIBLE_RESOLVE, out=out, workspace=workspace, footprint=1)
        for f in OUT:
            if f in ("depth", "index", "covered"):
                assert torch.equal(_bytes(out[f]), _bytes(full[f])), f
            else:
                assert (_np(out[f]).view(np.uint8) == 0x5a).all(), f                 # the resolve wrote its three outputs only
        workspace.fill_(0)                                                          # the test reads `depth`, not the workspace
        _raw(dev, p, k, c2w, height, width, m, hip.FIELD_VISIBLE_TEST, out=out, workspace=None, footprint=1)
        for f in OUT:
            assert torch.equal(_bytes(out[f]), _bytes(full[f])), f


def test_seven_calls_and_two_replays_of_a_capture_give_equal_bytes(dev):
    from neural_jacobian_field_amd.field_volume import FieldView, visible_rows
    rng = np.random.default_rng(11)
    k, c2w = _cameras(2)
    height, width = 12, 16
    pts = _cloud(rng, k, c2w, 2, 4097, height, width, reach=1.0)                      # 4,097 rows on 192 pixels: crowded
    p = _t(dev, pts)
    view = FieldView(_t(dev, k), _t(dev, c2w), height, width, footprint=2, tolerance=0.02)
    first = visible_rows(p, view)
    assert int(first.covered.min()) > 150 and int(first.visible.min()) > 20
    for _ in range(6):
        again = visible_rows(p, view)
        for f in OUT:
            assert torch.equal(_bytes(getattr(again, f)), _bytes(getattr(first, f))), f
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = visible_rows(p, view)
    for f in OUT:
        getattr(out, f).view(torch.uint8).fill_(0x77)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for f in OUT:
        assert torch.equal(_bytes(getattr(out, f)), _bytes(getattr(first, f))), f


# ---- 3. properties --------------------------------------------------------------------------------------------------------------------------
def test_a_permutation_of_the_rows_leaves_the_depth_and_maps_the_index(dev):
    from neural_jacobian_field_amd.field_volume import FieldView, visible_rows
    rng = np.random.default_rng(13)
    k, c2w = _cameras(3)
    height, width, n = 48, 64, 4097
    pts = _cloud(rng, k, c2w, 1, n, height, width, dirty=False)
    perm = rng.permutation(n)
    view = FieldView(_t(dev, k), _t(dev, c2w), height, width, footprint=1, tolerance=0.05)
    a, b = visible_rows(_t(dev, pts[0]), view), visible_rows(_t(dev, pts[0][perm]), view)
    assert torch.equal(_bytes(a.depth), _bytes(b.depth)) and torch.equal(a.covered, b.covered) and torch.equal(a.visible, b.visible)
    assert torch.equal(a.seen[0][_t(dev, perm)], b.seen[0])
    ia, ib, depth, z = _np(a.index[0]), _np(b.index[0]), _np(a.depth[0]), _np(a.z[0])
    for v in range(3):
        values, times = np.unique(z[v][np.isfinite(z[v])], return_counts=True)
        won = ia[v] >= 0
        untied = won & (times[np.searchsorted(values, depth[v]).clip(0, values.size - 1)] == 1)
        assert untied.sum() > 1000 and (perm[ib[v][untied]] == ia[v][untied]).all()
        assert (z[v][ia[v][won]] == depth[v][won]).all()


def test_the_depth_image_goes_back_through_depth_points(dev):
    """``FieldVisibility.depth[m]`` is a ``depth`` of ``depth_points(kind="z")`` with the same cameras: a pixel with a winner gives
    the point on the ray of the pixel's centre at the winner's z, an empty pixel none."""
    from neural_jacobian_field_amd.field_volume import FieldView, depth_points, visible_rows
    rng = np.random.default_rng(17)
    k, c2w = _cameras(3)
    height, width = 48, 64
    pts = _cloud(rng, k, c2w, 1, 4097, height, width)
    vis = visible_rows(_t(dev, pts[0]), FieldView(_t(dev, k), _t(dev, c2w), height, width, footprint=1))
    cloud = depth_points(vis.depth[0], _t(dev, k), _t(dev, c2w), kind="z")
    depth = _np(vis.depth[0])
    won = (depth > 0).reshape(3, -1)
    back = _np(cloud.points).reshape(3, height * width, 3)
    assert int(cloud.kept.sum()) == int(won.sum()) == int(vis.covered.sum()) and (np.isfinite(back).all(axis=2) == won).all()
    ref = S.pinhole_points(depth, k, c2w, "z")
    assert np.abs(back[won] - ref[won]).max() <= 1e-5
    again = V.project(back.reshape(1, -1, 3), k, c2w, height, width)               # and it projects into its own pixel again
    for v in range(3):
        rows = np.flatnonzero(won[v])
        assert (again["pixel"][0, v][v * height * width + rows] == rows).all()
        assert np.abs(again["z"][0, v][v * height * width + rows] - depth[v].reshape(-1)[rows]).max() <= 1e-5


# ---- 4. the registrations ---------------------------------------------------------------------------------------------------------------------
def _same_registration(a, b):
    from test_field_nearest_gpu import FIT, HISTORY, NEAR
    for f in FIT:
        assert torch.equal(_bytes(getattr(a.fit, f)), _bytes(getattr(b.fit, f))), f
    for f in NEAR:
        assert torch.equal(_bytes(getattr(a.matches, f)), _bytes(getattr(b.matches, f))), f
    for f in HISTORY:
        assert torch.equal(_bytes(getattr(a, f)), _bytes(getattr(b, f))), f


def _visible(s, observed, cells, reach, view, **kw):
    from neural_jacobian_field_amd.field_volume import register_commands_visible
    count = None if s.count is None else torch.tensor([s.count], dtype=torch.int32, device=s.dev)
    return register_commands_visible(s.tw, _t(s.dev, s.xyz), _t(s.dev, s.labels), observed, cells, reach, view, joints=s.joints, tree=s.tree,
                                     count=count, **kw)


def test_register_commands_visible_is_the_loop_of_its_public_pieces(dev):
    """Pose, ``visible_rows`` of the posed rows, ``nearest_points`` on the culled rows, ``solve_commands``: equal bytes in the fit,
    the matches and the four histories, for M = 2 starts and two cameras; ``register_commands`` itself returns what it did."""
    from neural_jacobian_field_amd.field_volume import (FieldRegistration, FieldView, FieldVisibleRegistration, nearest_points, part_poses,
                                                       solve_commands, visible_rows)
    chain = Scene(dev, J.chain())
    k, c2w = _cameras(2)
    planted = np.float32([[0.25, -0.2, 0.0]])
    rng = np.random.default_rng(19)
    observed = _t(dev, chain.targets(planted)[0][rng.permutation(272)])
    cells, reach = _scene_cells(chain.scene), 4 * chain.scene["step"][0]
    view = FieldView(_t(dev, k), _t(dev, c2w), 24, 32, footprint=1, tolerance=0.02)
    init = torch.tensor([[0.0, 0.0, 0.0], [0.3, 0.1, 0.0]], device=dev)
    reg = _visible(chain, observed, cells, reach, view, rounds=4, iterations=2, reg=1e-6, init=init)
    assert isinstance(reg, FieldVisibleRegistration) and reg.visible_history.shape == (4, 2) and reg.visible_history.dtype == torch.int32
    xyz, labels, u, history = _t(dev, chain.xyz), _t(dev, chain.labels), init, []
    count = None if chain.count is None else torch.tensor([chain.count], dtype=torch.int32, device=dev)
    for _ in range(4):
        posed = part_poses(chain.tw, u, joints=chain.joints, tree=chain.tree).apply(xyz, labels, count=count)
        seen = visible_rows(posed, view, labels=labels, count=count)
        near = nearest_points(seen.culled, observed, cells, reach, labels=labels, count=count)
        fit = solve_commands(chain.tw, xyz, labels, near.matched, joints=chain.joints, tree=chain.tree, count=count, init=u, iterations=2,
                             reg=1e-6)
        history.append((fit.commands.clone(), fit.cost.clone(), near.found.clone(), seen.visible.clone()))
        u = fit.commands
    loop = FieldVisibleRegistration(fit, near, *[torch.stack([h[i] for h in history]) for i in range(4)])
    _same_registration(reg, loop)
    assert torch.equal(reg.visible_history, loop.visible_history) and 0 < int(reg.visible_history.min()) <= int(reg.visible_history.max()) < 272
    assert (reg.found_history <= reg.visible_history).all()                          # a hidden row is free
    plain = _register(chain, observed, cells, reach, rounds=4, iterations=2, reg=1e-6, init=init)
    assert type(plain) is FieldRegistration and not hasattr(plain, "visible_history")


def test_the_whole_shell_registers_to_a_depth_image(dev):
    """Section 22's scene with ALL 878 rows of the shell: ``register_commands_visible`` converges, ``register_commands`` matches
    rows of the far side to the near side."""
    from neural_jacobian_field_amd.field_volume import FieldView, depth_points
    chain = Scene(dev, J.chain())
    k, c2w = _camera()
    xyz, labels = _shell(chain.scene, SHELL_MODEL)
    assert xyz.shape[0] == 878
    s = Scene(dev, chain.scene, given=(chain.tw, chain.joints, chain.tree, xyz, labels))
    fine = Scene(dev, chain.scene, given=(chain.tw, chain.joints, chain.tree, *_shell(chain.scene, SHELL_SEEN)))
    planted = np.float32([[ANGLES[0] / 0.7, ANGLES[1] / 1.3, 0.0]])
    depth = _z_buffer(fine.targets(planted)[0], k[0], c2w[0], HEIGHT, WIDTH)[None]
    cloud = depth_points(_t(dev, depth), _t(dev, k), _t(dev, c2w), kind="z", max_jump=MAX_JUMP)
    cells, reach = _scene_cells(chain.scene), 4 * chain.scene["step"][0]
    assert abs(reach - 0.4) < 1e-6
    view = FieldView(_t(dev, k), _t(dev, c2w), HEIGHT, WIDTH, footprint=1, tolerance=0.01)
    reg = _visible(s, cloud.points[0], cells, reach, view, rounds=ROUNDS, iterations=3)
    plain = _register(s, cloud.points[0], cells, reach, rounds=ROUNDS, iterations=3)
    history = []
    want = N.register(s.twists, s.xyz, s.labels, _np(cloud.points[0]), reach, s.parts, s.jd, s.td, rounds=ROUNDS, iterations=3,
                      search=V.cull(k, c2w, HEIGHT, WIDTH, 1, 0.01, history=history))
    d_got, d_plain, d_want = (float(np.abs(u - planted).max()) for u in (_np(reg.fit.commands), _np(plain.fit.commands), want["fit"]["commands"]))
    apart = float(np.abs(_np(reg.fit.commands) - want["fit"]["commands"]).max())
    print(f"878 rows: |u - planted| with the cull {d_got:.3e} (restatement {d_want:.3e}, |device - restatement| {apart:.3e}), without "
          f"{d_plain:.3e}; visible {reg.visible_history[:, 0].tolist()} (restatement {[int(h[0]) for h in history]}), found "
          f"{reg.found_history[:, 0].tolist()} and {plain.found_history[:, 0].tolist()}")
    assert reg.visible_history.shape == (ROUNDS, 1) and reg.visible_history.dtype == torch.int32
    assert not reg.fit.status.any()
    assert d_got <= CONVERGED                             # the cull makes the whole shell register
    assert _np(reg.visible_history).tolist() == np.stack(history).tolist()          # the restatement's counts, exactly
    assert d_got <= max(2.0 * d_want, 1e-6)               # test_field_normals_gpu's bound for the device against the restatement
    assert d_plain > 4 * CONVERGED                        # without it the far side is matched to the near side
    # the metric form: with the identity as every point's information it is the same registration
    identity = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], device=dev).expand(cloud.points.shape[1], 6).contiguous()
    metric = _visible(s, cloud.points[0], cells, reach, view, observed_information=identity, rounds=ROUNDS, iterations=3)
    d_metric = float(np.abs(_np(metric.fit.commands) - planted).max())
    print(f"metric form with the identity: |u - planted| {d_metric:.3e}, visible {metric.visible_history[:, 0].tolist()}")
    assert d_metric <= CONVERGED and metric.visible_history.shape == (ROUNDS, 1)
