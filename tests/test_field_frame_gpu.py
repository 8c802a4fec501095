"""GPU tests of the match of posed rows to a depth frame by projection (field_volume.frame_matches / register_commands_frame;
njf_field_frame) against the numpy restatement of its semantics (tests/field_frame_restatement.py), in two
layers, as section 24's are, so that exactness is asked only where it can hold.

Layer 1, the projection: ``pixel`` and ``z`` of the entry equal ``visible_rows``' bytes on the same points -- both call one device
function, and ``visible_rows`` is held to the float64 pinhole model by its own tests.

Layer 2, everything else, from the device's OWN ``pixel`` and ``z`` and its own fp32 world-to-camera matrices: state, states, index,
distance2, matched and found equal the restatement byte for byte, on outputs filled with two different sentinels.

A third check needs no restatement: where the window is the whole image, the match is ``nearest_points``' on the same cloud.

End to end (the last two tests): the scene of section 22 with ALL 878 shell rows, without and with a plate in front of the distal
link, within the bounds of tests/test_field_frame_cpu.py.  Measured on an MI355X, |u - planted|: 3.945e-2 at reach 4 and 8 (the
restatement's figure, and the commands of ``register_commands_visible`` on the device in every bit), 2.176e-1 at reach 1; behind
the plate 6.247e-2 (restatement 6.247e-2), 5.658e-1 with ``keep_hidden``, 5.582e-1 by the cell-list route; the device's ``pixel``
differs from the float64 model's on 0 of 878 rows.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_frame_restatement as R
import field_joints_restatement as J
import field_visible_restatement as V
from test_field_commands_gpu import Scene
from test_field_frame_cpu import COMMANDS, K1, _centres, occluded, restated_frame_registration
from test_field_nearest_gpu import FIT, HISTORY, NEAR, _scene_cells
from test_field_normals_gpu import _shell
from test_field_visible_gpu import _cameras, _cloud, _visible
from test_field_voxels_gpu import ANGLES, CONVERGED, HEIGHT, MAX_JUMP, ROUNDS, SHELL_MODEL, SHELL_SEEN, WIDTH, _camera, _z_buffer

pytestmark = pytest.mark.gpu

F32 = np.float32
ROWS = (1, 63, 64, 65, 257, 4097)
IMAGES = ((1, 1), (1, 7), (5, 3), (48, 64))
PROBLEMS = ((1, 1, 1, 1), (3, 3, 3, 3), (3, 3, 1, 3), (1, 3, 3, 1), (3, 3, 1, 1))            # (V, M, Mq, Mo)
REACHES = (0, 1, 4, 8)
TOLERANCES = (0.0, 0.05, 0.3)


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


def _frames(dev, rng, k, c2w, scenes, height, width):
    """[scenes, V H W, 3] on the device: ``depth_points`` of random depths in [1, 3], about a third of the pixels zero."""
    from neural_jacobian_field_amd.field_volume import depth_points
    views = k.shape[0]
    depth = rng.uniform(1.0, 3.0, (scenes * views, height, width)).astype(F32)
    depth[rng.random(depth.shape) < 1 / 3] = 0.0
    cloud = depth_points(_t(dev, depth), _t(dev, np.tile(k, (scenes, 1, 1))), _t(dev, np.tile(c2w, (scenes, 1, 1))), kind="z",
                         views_per_scene=views)
    assert cloud.points.shape == (scenes, views * height * width, 3) and int(cloud.kept.sum()) == int((depth > 0).sum())
    return cloud.points


def _outputs(dev, m, views, n, fill=None):
    from neural_jacobian_field_amd import hip
    shapes = dict(pixel=(m, views, n), z=(m, views, n), state=(m, views, n), index=(m, n), distance2=(m, n), matched=(m, n, 3), found=(m,),
                  states=(m, hip.FIELD_FRAME_STATES))
    out = {f: torch.empty(shapes[f], dtype=dtype, device=dev) for f, dtype in hip.FIELD_FRAME_OUTPUTS}
    if fill is not None:
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
    return out


def _raw(dev, points, frame, k, w2c, height, width, max_distance, m, phase, fill=None, **kw):
    """hip.field_frame on sentinel-filled outputs of the test's own; a dict of numpy arrays."""
    from neural_jacobian_field_amd import hip
    out = _outputs(dev, m, k.shape[0], points.shape[1], fill)
    hip.field_frame(points, frame, _t(dev, k), w2c, height, width, max_distance, out, m, phase=phase, **kw)
    return {f: _np(t) for f, t in out.items()}


def _check(dev, pts, frame, k, c2w, height, width, max_distance, m, reach, tolerance, keep, near=0.0, count=None, labels=None, what=""):
    """Two calls on outputs filled with different sentinels through both layers; the public function where it takes the case."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.field_volume import FieldView, frame_matches, visible_rows
    p, c, l = _t(dev, pts), (None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)), _t(dev, labels)
    w2c = hip.inverse(_t(dev, c2w))
    view = FieldView(_t(dev, k), _t(dev, c2w), height, width, near=near)
    vis = visible_rows(p, view, labels=l, count=c)                                  # [Mq, V, n]
    mq, read = pts.shape[0], V.read_rows(pts, count, labels)
    want = None
    for form, fill in (("first", 0x5a), ("second", 0xa5)):
        phase = hip.FIELD_FRAME_MATCH | (hip.FIELD_FRAME_KEEP_HIDDEN if keep else 0)
        got = _raw(dev, p, frame, k, w2c, height, width, max_distance, m, phase, fill=fill, count=c, labels=l, reach=reach, near=near,
                   tolerance=tolerance)
        for i in range(m):                                                          # layer 1: visible_rows' bytes
            q = 0 if mq == 1 else i
            assert got["pixel"][i].tobytes() == _np(vis.pixel[q]).tobytes(), (what, form, "pixel")
            assert got["z"][i].tobytes() == _np(vis.z[q]).tobytes(), (what, form, "z")
        if want is None:                                                            # (layer 1 holds both calls to the same pixel and z)
            want = R.finish(pts, _np(frame), got["pixel"][:mq].astype(np.int64), got["z"][:mq], read, _np(w2c), m, height, width,
                            max_distance, reach, tolerance, keep)
        for f in R.OUT:                                                             # layer 2: the restatement's bytes
            assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, form, f, got[f].dtype, got[f].shape)
            differ = int((got[f].view(np.uint8) != want[f].view(np.uint8)).sum())
            assert differ == 0, (what, form, f, differ)
    if max(mq, frame.shape[0]) == m:
        public = frame_matches(p if mq > 1 else p[0], frame if frame.shape[0] > 1 else frame[0], view, max_distance, reach=reach,
                               tolerance=tolerance, keep_hidden=keep, labels=l, count=c)
        for f in R.OUT:
            assert _np(getattr(public, f)).tobytes() == want[f].tobytes(), (what, f, "frame_matches")
    return want


# ---- 1. the two layers over the shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,width", IMAGES)
def test_every_output_equals_the_restatement(dev, height, width):
    rng = np.random.default_rng(1000 * height + width)
    case, seen, totals = 0, set(), np.zeros(R.STATES, np.int64)
    found = 0
    for n in ROWS:
        for views, m, mq, mo in PROBLEMS:
            reach, keep, tolerance = REACHES[case % 4], bool((case // 4) % 2), TOLERANCES[case % 3]
            case += 1
            k, c2w = _cameras(views)
            pts = _cloud(rng, k, c2w, mq, n, height, width)
            frame = _frames(dev, rng, k, c2w, mo, height, width)
            count = None if case % 3 else max(n - 3, 0)
            labels = None if case % 4 or n < 8 else np.where(rng.random(n) < 0.1, -1, rng.integers(0, 3, n)).astype(np.int32)
            want = _check(dev, pts, frame, k, c2w, height, width, 0.7, m, reach, tolerance, keep, count=count, labels=labels,
                          what=f"{height} x {width}, n {n}, V {views}, M {m}, Mq {mq}, Mo {mo}, reach {reach}, keep {keep}")
            assert (want["states"].sum(axis=1) == views * n).all()
            seen.add((reach, keep))
            totals += want["states"].sum(axis=0)
            found += int(want["found"].sum())
    print(f"{height} x {width}: {case} cases, states {totals.tolist()}, {found} rows matched")
    assert seen == {(r, kh) for r in REACHES for kh in (False, True)}
    assert totals[[R.OUTSIDE, R.NO_RETURN, R.IN_FRONT, R.BEHIND]].all() and found > 0


# ---- 2. against existing device code --------------------------------------------------------------------------------------------------------
def test_a_window_over_the_whole_image_is_the_cell_lists_nearest_point(dev):
    """5 x 3, one view, reach 4, ``keep_hidden``: every inside row searches the whole frame, as ``nearest_points`` does."""
    from neural_jacobian_field_amd.field_volume import FieldView, cell_grid, frame_matches, nearest_points
    rng = np.random.default_rng(31)
    k, c2w = _cameras(1)
    height, width, n = 5, 3, 257
    for mq, mo in ((1, 1), (3, 1), (1, 3), (3, 3)):
        pts = _cloud(rng, k, c2w, mq, n, height, width)
        frame = _frames(dev, rng, k, c2w, mo, height, width)
        p = _t(dev, pts)
        view = FieldView(_t(dev, k), _t(dev, c2w), height, width)
        got = frame_matches(p, frame, view, 1.5, reach=4, keep_hidden=True)
        cloud = _np(frame).reshape(-1, 3)
        lower, upper = np.nanmin(cloud, axis=0) - 0.5, np.nanmax(cloud, axis=0) + 0.5
        near = nearest_points(p, frame, cell_grid(lower.tolist(), upper.tolist(), 0.25), 1.5)
        inside = got.pixel[:, 0] >= 0                                               # [M, n]
        assert 20 < int(inside.sum()) < inside.numel() and int(got.found.sum()) > 5
        for f in NEAR[:3]:
            a, b = getattr(got, f)[inside], getattr(near, f)[inside]
            assert torch.equal(_bytes(a), _bytes(b)), (f, mq, mo)
        assert (got.index[~inside] == -1).all()


# ---- 3. edge rows ---------------------------------------------------------------------------------------------------------------------------
def test_rows_that_are_not_read_behind_the_camera_at_near_and_off_the_image(dev):
    """An identity camera and coordinates that are exact in fp32: the restatement from the float64 model holds byte for byte."""
    from neural_jacobian_field_amd import hip
    k = K1.astype(F32)
    w2c = np.eye(4, dtype=F32)[None]
    near = 0.25
    pts = F32([[-0.375, -0.375, 1.0],      # 0: pixel (0, 0), in front of the plane at 1.5
               [-0.375, -0.375, 2.0],      # 1: pixel (1, 1), behind it
               [0.0, 0.0, -1.0],           # 2: behind the camera
               [0.0, 0.0, 0.25],           # 3: z == near: not projectable
               [np.nan, 0.0, 1.0],         # 4: not finite
               [0.625, 0.125, 1.0],        # 5: col 4 of 4: just off the right edge
               [0.125, 0.125, 0.5],        # 6: label -1
               [0.1875, 0.1875, 1.5],      # 7: pixel (2, 2), on the plane, at the pixel's centre
               [0.125, 0.125, 1.0],        # 8: from the count on
               [0.125, 0.125, 0.75]])[None]
    labels = np.int32([0, 0, 0, 0, 0, 0, -1, 2, 0, 0])
    frame = _centres(4, 4, 1.5)
    assert frame[10].tolist() == [0.1875, 0.1875, 1.5]
    kw = dict(count=torch.tensor([8], dtype=torch.int32, device=dev), labels=_t(dev, labels), near=near, tolerance=0.125)
    for reach in (0, 1):
        for keep in (False, True):
            want = R.matches(pts, frame, k, w2c, 4, 4, 1.0, reach=reach, tolerance=0.125, near=near, keep_hidden=keep, count=8, labels=labels)
            phase = hip.FIELD_FRAME_MATCH | (hip.FIELD_FRAME_KEEP_HIDDEN if keep else 0)
            got = _raw(dev, _t(dev, pts), _t(dev, frame[None]), k, _t(dev, w2c), 4, 4, 1.0, 1, phase, fill=0x5a, reach=reach, **kw)
            for f in R.OUT:
                assert got[f].tobytes() == want[f].tobytes(), (f, reach, keep)
            assert want["pixel"][0, 0].tolist() == [0, 5, -1, -1, -1, -1, -1, 10, -1, -1]
            assert want["state"][0, 0].tolist() == [R.IN_FRONT, R.BEHIND, 0, 0, 0, 0, 0, R.ON, 0, 0]
            assert want["z"][0, 0, :4].tolist() == [1.0, 2.0, -1.0, 0.25] and np.isnan(want["z"][0, 0, [4, 6, 8, 9]]).all()
            assert want["z"][0, 0, 5] == 1.0                                        # read and projectable, with no pixel of its own
            # rows 0 and 1 lie as far from the points of pixels 0, 1, 4 and 5: with reach 1 the tie goes to frame row 0
            assert want["index"][0].tolist() == [0, (5 if reach == 0 else 0) if keep else -1, -1, -1, -1, -1, -1, 10, -1, -1]
            assert want["states"].tolist() == [[7, 0, 1, 1, 1]] and want["found"].tolist() == [3 if keep else 2]
            assert want["distance2"][0, 7] == 0.0 and want["matched"][0, 7].tobytes() == frame[10].tobytes()


def test_4097_rows_in_one_pixel_and_a_frame_of_nan(dev):
    rng = np.random.default_rng(5)
    k, c2w = _cameras(1)
    height, width, n = 5, 3, 4097
    k64, c64 = k.astype(np.float64), c2w.astype(np.float64)
    z = rng.choice([1.25, 1.5, 2.0, 2.75], n)
    xy = np.stack([rng.choice([1.3, 1.5, 1.7], n) / width, rng.choice([2.4, 2.6], n) / height, np.ones(n)], axis=1)
    pts = ((xy @ np.linalg.inv(k64[0]).T * z[:, None]) @ c64[0, :3, :3].T + c64[0, :3, 3]).astype(F32)[None]
    frame = _frames(dev, rng, k, c2w, 1, height, width)
    frame[0, 2 * width + 1] = _t(dev, pts[0, 0])                                     # the own pixel holds row 0 itself
    for reach in (0, 2):
        want = _check(dev, pts, frame, k, c2w, height, width, 5.0, 1, reach, 0.05, True, what=f"one pixel, reach {reach}")
        assert (want["pixel"] == 2 * width + 1).all() and want["states"][0, [R.OUTSIDE, R.NO_RETURN]].tolist() == [0, 0]
        assert want["found"][0] == n and want["distance2"][0, 0] == 0.0 and want["index"][0, 0] == 2 * width + 1
        assert reach or (want["index"] == 2 * width + 1).all()
    empty = torch.full_like(frame, float("nan"))
    want = _check(dev, pts, empty, k, c2w, height, width, 5.0, 1, 8, 0.05, True, what="a frame of NaN")
    assert want["found"].tolist() == [0] and want["states"].tolist() == [[0, n, 0, 0, 0]] and (want["index"] == -1).all()
    mixed = _cloud(rng, k, c2w, 1, 257, height, width)
    want = _check(dev, mixed, empty, k, c2w, height, width, 5.0, 1, 4, 0.05, False, what="a frame of NaN, rows anywhere")
    assert want["found"].tolist() == [0] and want["states"][0, 2:].tolist() == [0, 0, 0] and want["states"][0, :2].all()


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------------
def test_seven_calls_and_two_replays_of_a_capture_give_equal_bytes(dev):
    from neural_jacobian_field_amd.field_volume import FieldView, frame_matches
    rng = np.random.default_rng(11)
    k, c2w = _cameras(2)
    height, width = 12, 16
    pts = _cloud(rng, k, c2w, 2, 4097, height, width, reach=1.0)
    frame = _frames(dev, rng, k, c2w, 1, height, width)
    p = _t(dev, pts)
    view = FieldView(_t(dev, k), _t(dev, c2w), height, width)
    first = frame_matches(p, frame, view, 0.7, reach=4)
    assert int(first.found.min()) > 100 and (first.states.sum(dim=1) == 2 * 4097).all()
    for _ in range(6):
        again = frame_matches(p, frame, view, 0.7, reach=4)
        for f in R.OUT:
            assert torch.equal(_bytes(getattr(again, f)), _bytes(getattr(first, f))), f
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = frame_matches(p, frame, view, 0.7, reach=4)
    for f in R.OUT:
        getattr(out, f).view(torch.uint8).fill_(0x77)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for f in R.OUT:
        assert torch.equal(_bytes(getattr(out, f)), _bytes(getattr(first, f))), f


# ---- 5. the registrations -------------------------------------------------------------------------------------------------------------------
def _frame_registration(s, frame, reach_distance, view, **kw):
    from neural_jacobian_field_amd.field_volume import register_commands_frame
    count = None if s.count is None else torch.tensor([s.count], dtype=torch.int32, device=s.dev)
    return register_commands_frame(s.tw, _t(s.dev, s.xyz), _t(s.dev, s.labels), frame, reach_distance, view, joints=s.joints, tree=s.tree,
                                   count=count, **kw)


def test_register_commands_frame_is_the_loop_of_its_public_pieces(dev):
    """Pose, ``visible_rows`` of the posed rows, ``frame_matches`` on the culled rows, ``solve_commands`` or its metric form: equal
    bytes in the fit, the matches and the five histories, for M = 2 starts and two cameras."""
    from neural_jacobian_field_amd.field_volume import (FieldFrameMatches, FieldFrameRegistration, FieldView, depth_points, frame_matches,
                                                       part_poses, solve_commands, solve_commands_metric, visible_rows)
    chain = Scene(dev, J.chain())
    k, c2w = _cameras(2)
    height, width = 24, 32
    view = FieldView(_t(dev, k), _t(dev, c2w), height, width, footprint=1, tolerance=0.02)
    xyz, labels = _t(dev, chain.xyz), _t(dev, chain.labels)
    count = None if chain.count is None else torch.tensor([chain.count], dtype=torch.int32, device=dev)
    planted = torch.tensor([[0.25, -0.2, 0.0]], device=dev)
    seen = visible_rows(part_poses(chain.tw, planted, joints=chain.joints, tree=chain.tree).apply(xyz, labels, count=count), view,
                        labels=labels, count=count)
    frame = depth_points(seen.depth[0], view.intrinsics, view.cam2world, kind="z", views_per_scene=2).points     # [1, 2 H W, 3]
    assert int(seen.covered.min()) > 20
    init = torch.tensor([[0.0, 0.0, 0.0], [0.3, 0.1, 0.0]], device=dev)
    reach_distance = 4 * chain.scene["step"][0]
    information = torch.rand(frame.shape[1], 6, device=dev) * 0.1 + torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], device=dev)
    for info in (None, information):
        kw = dict(reach=3, tolerance=0.05, keep_hidden=info is not None)
        reg = _frame_registration(chain, frame, reach_distance, view, observed_information=info, rounds=4, iterations=2, reg=1e-6, init=init,
                                  **kw)
        assert isinstance(reg, FieldFrameRegistration) and isinstance(reg.matches, FieldFrameMatches)
        assert reg.states_history.shape == (4, 2, 5) and reg.states_history.dtype == torch.int32
        u, history = init, []
        for _ in range(4):
            posed = part_poses(chain.tw, u, joints=chain.joints, tree=chain.tree).apply(xyz, labels, count=count)
            seen = visible_rows(posed, view, labels=labels, count=count)
            near = frame_matches(seen.culled, frame, view, reach_distance, labels=labels, count=count, **kw)
            if info is None:
                fit = solve_commands(chain.tw, xyz, labels, near.matched, joints=chain.joints, tree=chain.tree, count=count, init=u,
                                     iterations=2, reg=1e-6)
            else:
                rows = info[near.index.clamp_min(0).long()]
                fit = solve_commands_metric(chain.tw, xyz, labels, near.matched, rows, joints=chain.joints, tree=chain.tree, count=count,
                                            init=u, iterations=2, reg=1e-6)
            history.append((fit.commands.clone(), fit.cost.clone(), near.found.clone(), seen.visible.clone(), near.states.clone()))
            u = fit.commands
        for f in FIT:
            assert torch.equal(_bytes(getattr(reg.fit, f)), _bytes(getattr(fit, f))), f
        for f in R.OUT:
            assert torch.equal(_bytes(getattr(reg.matches, f)), _bytes(getattr(near, f))), f
        for i, f in enumerate(HISTORY + ("visible_history", "states_history")):
            assert torch.equal(_bytes(getattr(reg, f)), _bytes(torch.stack([h[i] for h in history]))), f
        assert 0 < int(reg.found_history.min()) and (reg.found_history <= reg.visible_history).all()
        assert (reg.states_history.sum(dim=2) == 2 * chain.xyz.shape[0]).all()


def _shell_scene(dev):
    chain = Scene(dev, J.chain())
    k, c2w = _camera()
    xyz, labels = _shell(chain.scene, SHELL_MODEL)
    assert xyz.shape[0] == 878
    s = Scene(dev, chain.scene, given=(chain.tw, chain.joints, chain.tree, xyz, labels))
    fine = Scene(dev, chain.scene, given=(chain.tw, chain.joints, chain.tree, *_shell(chain.scene, SHELL_SEEN)))
    planted = np.float32([[ANGLES[0] / 0.7, ANGLES[1] / 1.3, 0.0]])
    depth = _z_buffer(fine.targets(planted)[0], k[0], c2w[0], HEIGHT, WIDTH)[None]
    return chain, s, k, c2w, planted, depth


def _restatement_scene(s):
    return dict(twists=s.twists, xyz=s.xyz, labels=s.labels, parts=s.parts, joints=s.jd, tree=s.td, step=s.scene["step"][0])


def _pixel_differences(s, frame, view, k, c2w, commands):
    """Rows on which the device's own pixel differs from the float64 model's, over the rows posed at ``commands``."""
    from neural_jacobian_field_amd.field_volume import frame_matches
    posed = s.targets(np.float32(commands))
    got = _np(frame_matches(_t(s.dev, posed), frame, view, 0.4, labels=_t(s.dev, s.labels)).pixel)
    read = V.read_rows(posed, None, s.labels)
    want = np.where(read[:, None], V.project(posed, k, c2w, HEIGHT, WIDTH)["pixel"], -1)
    return int((got != want).sum()), int(got.size)


def test_the_whole_shell_registers_to_the_frame_like_the_cell_list_route(dev):
    """Section 22's scene with ALL 878 rows and no occluder: a window of reach 4 or 8 covers the displacement and the frame route
    converges as the cell-list route does; reach 1 does not.  Measured on an MI355X: see DESIGN.md section 26."""
    from neural_jacobian_field_amd.field_volume import FieldView, depth_points
    chain, s, k, c2w, planted, depth = _shell_scene(dev)
    cloud = depth_points(_t(dev, depth), _t(dev, k), _t(dev, c2w), kind="z", max_jump=MAX_JUMP)
    frame = cloud.points[0]
    view = FieldView(_t(dev, k), _t(dev, c2w), HEIGHT, WIDTH, footprint=1, tolerance=0.01)
    cells = _visible(s, frame, _scene_cells(chain.scene), 0.4, view, rounds=ROUNDS, iterations=3)
    d_cells = float(np.abs(_np(cells.fit.commands) - planted).max())
    errors = {}
    for reach in (1, 4, 8):
        reg = _frame_registration(s, frame, 0.4, view, reach=reach, rounds=ROUNDS, iterations=3)
        want = restated_frame_registration(_restatement_scene(s), k, c2w, _np(frame), reach=reach)
        errors[reach] = float(np.abs(_np(reg.fit.commands) - planted).max())
        d_want = float(np.abs(want["fit"]["commands"] - planted).max())
        print(f"reach {reach}: |u - planted| {errors[reach]:.3e} (restatement {d_want:.3e}, cell-list route on the device {d_cells:.3e}); "
              f"found {reg.found_history[:, 0].tolist()}, visible {reg.visible_history[:, 0].tolist()}, states of the last round "
              f"{reg.states_history[-1, 0].tolist()} (restatement {want['states_history'][-1, 0].tolist()})")
        assert not reg.fit.status.any() and (reg.states_history.sum(dim=2) == 878).all()
        if reach > 1:
            assert errors[reach] <= CONVERGED
            print(f"  the commands of the cell-list route in every bit: {torch.equal(_bytes(reg.commands_history), _bytes(cells.commands_history))}")
    assert errors[1] > 4 * CONVERGED and d_cells <= CONVERGED
    differ = [_pixel_differences(s, frame, view, k, c2w, u) for u in (planted, [[0.0, 0.0, 0.0]])]
    print(f"rows whose pixel differs from the float64 model's: {[d[0] for d in differ]} of {differ[0][1]}")
    # explained(): the planted command agrees best with the frame
    from neural_jacobian_field_amd.field_volume import frame_matches, visible_rows
    share = []
    for u in (planted[0], (0.0, 0.0, 0.0)) + COMMANDS:
        posed = _t(dev, s.targets(np.float32([u])))
        seen = visible_rows(posed, view, labels=_t(dev, s.labels))
        got = frame_matches(seen.culled, frame, view, 0.4, reach=4, tolerance=0.05, labels=_t(dev, s.labels))
        share.append(float(got.explained()[0]))
    print("explained:", [f"{v:.3f}" for v in share])
    assert all(share[0] > v for v in share[1:])


def test_rows_behind_a_plate_are_freed_by_the_frame(dev):
    """The same scene with a plate 0.15 in front of the distal link: the frame route stays within twice the bound, ``keep_hidden``
    and the cell-list route are pulled onto the plate.  Measured on an MI355X: see DESIGN.md section 26."""
    from neural_jacobian_field_amd.field_volume import FieldView, depth_points
    chain, s, k, c2w, planted, depth = _shell_scene(dev)
    plated, want_frame, hidden = occluded(depth, k, c2w)
    cloud = depth_points(_t(dev, plated), _t(dev, k), _t(dev, c2w), kind="z", max_jump=MAX_JUMP)
    frame = cloud.points[0]
    assert hidden == 192 and int(cloud.kept[0]) == 1021
    assert (np.isfinite(_np(frame)).all(axis=1) == np.isfinite(want_frame).all(axis=1)).all()
    view = FieldView(_t(dev, k), _t(dev, c2w), HEIGHT, WIDTH, footprint=1, tolerance=0.01)
    errors = {}
    for key, kw in (("reach 4, tolerance 0.01", dict(reach=4, tolerance=0.01)), ("reach 8, tolerance 0.05", dict(reach=8, tolerance=0.05)),
                    ("keep_hidden", dict(reach=4, keep_hidden=True))):
        reg = _frame_registration(s, frame, 0.4, view, rounds=ROUNDS, iterations=3, **kw)
        want = restated_frame_registration(_restatement_scene(s), k, c2w, _np(frame), **kw)
        errors[key] = float(np.abs(_np(reg.fit.commands) - planted).max())
        print(f"{key}: |u - planted| {errors[key]:.3e} (restatement {float(np.abs(want['fit']['commands'] - planted).max()):.3e}); found "
              f"{reg.found_history[:, 0].tolist()}, states of the last round {reg.states_history[-1, 0].tolist()} (restatement "
              f"{want['states_history'][-1, 0].tolist()})")
        assert not reg.fit.status.any()
    cells = _visible(s, frame, _scene_cells(chain.scene), 0.4, view, rounds=ROUNDS, iterations=3)
    d_cells = float(np.abs(_np(cells.fit.commands) - planted).max())
    print(f"cell-list route with the cull: |u - planted| {d_cells:.3e}")
    assert errors["reach 4, tolerance 0.01"] <= 2 * CONVERGED and errors["reach 8, tolerance 0.05"] <= 2 * CONVERGED
    assert errors["keep_hidden"] > 4 * CONVERGED and d_cells > 4 * CONVERGED
    differ = [_pixel_differences(s, frame, view, k, c2w, u) for u in (planted, [[0.0, 0.0, 0.0]])]
    print(f"rows whose pixel differs from the float64 model's: {[d[0] for d in differ]} of {differ[0][1]}")
