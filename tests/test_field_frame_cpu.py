"""Host-side tests of the match of posed rows to a depth frame by projection (field_volume.frame_matches / register_commands_frame
/ cloud_registration_frame; njf_field_frame): the numpy restatement (tests/field_frame_restatement.py) --
the states at equality of the tolerance rule, a window clipped by hand, the ties, the rows that are not read, a frame of NaN,
``keep_hidden``, ``explained()`` --, the signatures, every argument check, raised before any device work (there is no GPU here), the
C ABI's symbol and return codes, and the conditions the GPU tests rely on: the numpy registrations of the section-22 scene.

The bounds are section 22's ``CONVERGED = 0.05`` (derived there) and, for the occluded scene, twice that: a quarter of the body,
most of it on the distal link, contributes no rows.  Measured here, |u - planted|: (a) no occluder 3.945e-2 with reach 4 or 8 (175
rows found in every round, the commands of the cell-list route bit for bit), 7.697e-2 with reach 2, 2.176e-1 with reach 1 (161
rows); (b) behind a plate 0.15 in front of the distal link 6.247e-2 with reach 4 or 8 and tolerance 0.01 to 0.05 (ON 117, BEHIND
30, NO_RETURN 28 in the last round), 5.658e-1 with ``keep_hidden``, 5.582e-1 by the cell-list route with the cull; (c) ON rows
167 / 141 / 107 / 123 / 95 at the planted command and four others."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_commands_restatement as F
import field_frame_restatement as R
import field_joints_restatement as J
import field_nearest_restatement as N
import field_visible_restatement as V
import field_voxels_restatement as S
from test_field_nearest_cpu import _cpu_arguments
from test_field_visible_cpu import _bad_views, _view, restated_registration, section_22_scene
from test_field_voxels_gpu import CONVERGED, HEIGHT, MAX_JUMP, ROUNDS, WIDTH, _camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 27
F32 = np.float32
K1 = np.array([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]])       # the unit pinhole: u = x / z + 1/2
EYE = np.eye(4)[None]
DEFAULT = object()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


def _centres(height, width, z=1.0):
    """fp32 [H W, 3]: the points of the pixel centres of the unit pinhole at depth z -- a frame of a plane."""
    r, c = np.divmod(np.arange(height * width), width)
    return np.stack([((c + 0.5) / width - 0.5) * z, ((r + 0.5) / height - 0.5) * z, np.full(r.shape, z)], axis=1).astype(F32)


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
def test_the_states_at_equality_of_the_tolerance_rule():
    # zo = 2 and tolerance 1/4: the slack 0.5 and every difference below are exact in fp32
    own = F32([[0, 0, 2.0]] * 8)
    z = F32([2.0, 2.5, np.nextafter(F32(2.5), F32(3)), 1.5, np.nextafter(F32(1.5), F32(1)), 2.25, np.nan, 2.0])
    pixel = np.int64([0, 0, 0, 0, 0, 0, 0, -1])
    got = R.states_of(pixel, z, own, np.eye(4, dtype=F32), 0.25).tolist()
    assert got == [R.ON, R.ON, R.BEHIND, R.ON, R.IN_FRONT, R.ON, R.ON, R.OUTSIDE]      # inclusive on both sides; a NaN compares false
    assert R.states_of(pixel, z, own, np.eye(4, dtype=F32), 0.0).tolist() == [R.ON, R.BEHIND, R.BEHIND, R.IN_FRONT, R.IN_FRONT, R.BEHIND,
                                                                               R.ON, R.OUTSIDE]
    # a tolerance that is not exact: the rule is the fp32 subtraction against the fp32 product, whatever they round to
    tol, zo = 0.01, F32(2.0)
    slack = F32(F32(tol) * zo)
    for at in (F32(zo + slack), F32(zo - slack)):
        for zc in (at, np.nextafter(at, F32(10)), np.nextafter(at, F32(-10))):
            want = R.IN_FRONT if F32(zo - zc) > slack else R.BEHIND if F32(zc - zo) > slack else R.ON
            assert R.states_of([0], F32([zc]), F32([[7, -3, 2.0]]), np.eye(4, dtype=F32), tol).tolist() == [want]
    assert R.states_of([0], F32([np.nextafter(F32(zo + slack), F32(10))]), own[:1], np.eye(4, dtype=F32), tol).tolist() == [R.BEHIND]
    assert R.states_of([0], F32([np.nextafter(F32(zo - slack), F32(-10))]), own[:1], np.eye(4, dtype=F32), tol).tolist() == [R.IN_FRONT]
    # no return: one coordinate that is not finite is enough; zo comes from the third row of w2c (here z' = 2 z + 1)
    assert R.states_of([0, 0, 0], F32([2, 2, 2]), F32([[np.nan, 0, 2], [0, np.inf, 2], [0, 0, -np.inf]]), np.eye(4, dtype=F32), 0.1).tolist() \
        == [R.NO_RETURN] * 3
    w = np.eye(4, dtype=F32)
    w[2] = [0, 0, 2, 1]
    assert R.camera_z(w, F32([[5, 6, 2.0]])).tolist() == [5.0]
    assert R.states_of([0, 0, 0], F32([5.0, 4.0, 6.0]), F32([[5, 6, 2.0]] * 3), w, 0.1).tolist() == [R.ON, R.IN_FRONT, R.BEHIND]


def test_a_window_clipped_by_hand_on_a_3_by_5_image():
    assert R.window(0, 0, 3, 5, 0) == [(0, 0)]
    assert R.window(0, 0, 3, 5, 1) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert R.window(2, 4, 3, 5, 2) == [(r, c) for r in (0, 1, 2) for c in (2, 3, 4)]
    assert R.window(1, 2, 3, 5, 8) == [(r, c) for r in range(3) for c in range(5)]
    # a plane at z = 1; the own pixel (0, 0) gave no point, and pixel (0, 3) holds the query itself
    frame = _centres(3, 5)
    query = frame[0].copy()
    frame[0], frame[3] = np.nan, query
    got = {reach: R.matches(query[None], frame, K1, EYE, 3, 5, 1.0, reach=reach) for reach in (0, 1, 2, 3)}
    assert all(g["pixel"].tolist() == [[[0]]] and g["state"].tolist() == [[[R.NO_RETURN]]] for g in got.values())
    assert got[0]["index"].tolist() == [[-1]] and got[0]["found"].tolist() == [0] and np.isnan(got[0]["matched"]).all()
    assert np.isinf(got[0]["distance2"]).all()
    for reach in (1, 2):                                  # (0, 1), 0.2 to the right, is closer than (1, 0), 1/3 below; (0, 3) is out of reach
        assert got[reach]["index"].tolist() == [[1]] and got[reach]["matched"][0, 0].tobytes() == frame[1].tobytes()
        d = query - frame[1]
        assert got[reach]["distance2"][0, 0] == F32(F32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    assert got[3]["index"].tolist() == [[3]] and got[3]["distance2"].tolist() == [[0.0]]
    assert R.matches(query[None], frame, K1, EYE, 3, 5, 0.19, reach=2)["found"].tolist() == [0]       # found, but beyond max_distance
    assert R.matches(query[None], frame, K1, EYE, 3, 5, 0.0, reach=3)["index"].tolist() == [[3]]      # d2 <= 0 * 0 is inclusive


def test_ties_go_to_the_lowest_frame_row_within_a_view_and_across_views():
    # 1 x 2: both pixels hold the same point; the row lies in pixel 1 and still gets row 0
    point = F32([[0.25, 0.0, 1.0]])
    frame = np.concatenate([point, point])
    got = R.matches(point, frame, K1, EYE, 1, 2, 1.0, reach=1)
    assert got["pixel"].tolist() == [[[1]]] and got["index"].tolist() == [[0]] and got["distance2"].tolist() == [[0.0]]
    assert R.matches(point, frame, K1, EYE, 1, 2, 1.0, reach=0)["index"].tolist() == [[1]]
    # two equal views of 1 x 1: the frame rows 0 and 1 tie; without a return in view 0 it is row 1
    k2, c2 = np.concatenate([K1, K1]), np.concatenate([EYE, EYE])
    got = R.matches(point, frame, k2, c2, 1, 1, 1.0, reach=0)
    assert got["index"].tolist() == [[0]] and got["state"].tolist() == [[[R.ON], [R.ON]]] and got["states"].tolist() == [[0, 0, 0, 2, 0]]
    frame[0] = np.nan
    got = R.matches(point, frame, k2, c2, 1, 1, 1.0, reach=0)
    assert got["index"].tolist() == [[1]] and got["state"].tolist() == [[[R.NO_RETURN], [R.ON]]]
    # equal distances to two different points: the lower row
    frame = F32([[0.25, 0.125, 1.0], [0.25, -0.125, 1.0]])
    assert R.matches(point, frame, K1, EYE, 1, 2, 1.0, reach=1)["index"].tolist() == [[0]]
    assert R.matches(point, frame[::-1].copy(), K1, EYE, 1, 2, 1.0, reach=1)["index"].tolist() == [[0]]


def test_rows_that_are_not_read_a_frame_of_nan_and_keep_hidden():
    frame = _centres(3, 3, 2.0)
    pts = F32([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 3.0], [np.nan, 0, 2.0], [0, 0, 2.0], [0, 0, 2.0], [0, 0, -1.0], [5.0, 0, 2.0]])
    labels = np.int32([0, 1, 2, 0, -1, 0, 0, 0])
    got = R.matches(pts, frame, K1, EYE, 3, 3, 10.0, reach=1, tolerance=0.1, count=7, labels=labels)
    # 0 on; 1 in front; 2 behind: not searched; 3 not finite, 4 of label -1: not read; 5 read; 6 behind the camera; 7 from the count on
    assert got["state"][0, 0].tolist() == [R.ON, R.IN_FRONT, R.BEHIND, R.OUTSIDE, R.OUTSIDE, R.ON, R.OUTSIDE, R.OUTSIDE]
    assert got["pixel"][0, 0].tolist() == [4, 4, 4, -1, -1, 4, -1, -1] and got["states"].tolist() == [[4, 0, 1, 2, 1]]
    assert np.isnan(got["z"][0, 0, [3, 4, 7]]).all() and got["z"][0, 0, [0, 1, 2, 5, 6]].tolist() == [2.0, 1.0, 3.0, 2.0, -1.0]
    assert got["index"].tolist() == [[4, 4, -1, -1, -1, 4, -1, -1]] and got["found"].tolist() == [3]
    assert np.isnan(got["matched"][0, [2, 3, 4, 6, 7]]).all() and np.isinf(got["distance2"][0, [2, 3, 4, 6, 7]]).all()
    assert got["distance2"][0, :2].tolist() == [0.0, 1.0]
    kept = R.matches(pts, frame, K1, EYE, 3, 3, 10.0, reach=1, tolerance=0.1, count=7, labels=labels, keep_hidden=True)
    assert kept["index"].tolist() == [[4, 4, 4, -1, -1, 4, -1, -1]] and kept["found"].tolist() == [4]
    assert kept["state"].tobytes() == got["state"].tobytes() and kept["states"].tobytes() == got["states"].tobytes()
    # off the image: read and projected, a z and no pixel
    off = R.matches(pts, frame, K1, EYE, 3, 3, 10.0, reach=8)
    assert off["pixel"][0, 0, 7] == -1 and off["z"][0, 0, 7] == 2.0 and off["state"][0, 0, 7] == R.OUTSIDE and off["index"][0, 7] == -1
    # a frame of NaN: nothing is found and every state is NO_RETURN or OUTSIDE; one frame for two problems
    empty = R.matches(np.stack([pts, pts[::-1]]), np.full((9, 3), np.nan, F32), K1, EYE, 3, 3, 10.0, reach=8)
    assert empty["found"].tolist() == [0, 0] and (empty["index"] == -1).all() and set(empty["state"].reshape(-1).tolist()) == {0, 1}
    assert empty["states"].tolist() == [[3, 5, 0, 0, 0]] * 2 and np.isnan(R.explained(empty["states"])).tolist() == [False, False]


def test_explained():
    assert R.explained([[5, 1, 1, 6, 9]]).tolist() == [0.75]
    assert np.isnan(R.explained([[5, 0, 0, 0, 3], [0, 0, 0, 0, 0]])).all()
    from neural_jacobian_field_amd.field_volume import FieldFrameMatches
    empty = torch.zeros(0)
    m = FieldFrameMatches(index=empty, distance2=empty, matched=empty, found=empty, state=empty,
                          states=torch.tensor([[5, 1, 1, 6, 9], [5, 0, 0, 0, 3], [0, 2, 0, 0, 0]], dtype=torch.int32), pixel=empty, z=empty)
    got = m.explained()
    assert got.dtype == torch.float64 and got.shape == (3,) and got[0] == 0.75 and torch.isnan(got[1]) and got[2] == 0.0


# ---- the interface ------------------------------------------------------------------------------------------------------------------------
def test_the_signatures():
    from neural_jacobian_field_amd import field_volume as fv
    from neural_jacobian_field_amd import hip
    params = inspect.signature(fv.frame_matches).parameters
    assert list(params) == ["points", "frame", "view", "max_distance", "reach", "tolerance", "keep_hidden", "labels", "count"]
    keywords = dict(reach=4, tolerance=0.02, keep_hidden=False, labels=None, count=None)
    assert {k: params[k].default for k in keywords} == keywords
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keywords)
    assert issubclass(fv.FieldFrameMatches, fv.FieldNearest)
    assert list(fv.FieldFrameMatches.__dataclass_fields__) == list(fv.FieldNearest.__dataclass_fields__) + ["state", "states", "pixel", "z"]
    assert [name for name, _ in hip.FIELD_FRAME_OUTPUTS] == list(R.OUT)
    assert list(fv.FieldView.__dataclass_fields__) == ["intrinsics", "cam2world", "height", "width", "footprint", "tolerance", "near"]
    # the registrations: register_commands_visible's arguments without the lattice and the observed count, the window behind the information
    for fn, base in ((fv.register_commands_frame, fv.register_commands_visible), (fv.cloud_registration_frame, fv.cloud_registration_visible)):
        params, visible = inspect.signature(fn).parameters, inspect.signature(base).parameters
        positional = [k for k, v in visible.items() if v.kind is v.POSITIONAL_OR_KEYWORD and k != "cells"]
        rest = {k: v.default for k, v in visible.items() if v.kind is v.KEYWORD_ONLY and k not in ("observed_information", "cells", "observed_count")}
        positional = [dict(observed="frame", visible_from="view").get(k, k) for k in positional]
        assert list(params) == positional + ["observed_information", "reach", "tolerance", "keep_hidden"] + list(rest)
        assert all(params[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and params[k].default is inspect.Parameter.empty for k in positional)
        added = dict(observed_information=None, reach=4, tolerance=0.02, keep_hidden=False)
        assert {k: params[k].default for k in added} == added and {k: params[k].default for k in rest} == rest
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(added) + list(rest))
    assert issubclass(fv.FieldFrameRegistration, fv.FieldVisibleRegistration)
    assert list(fv.FieldFrameRegistration.__dataclass_fields__) == list(fv.FieldVisibleRegistration.__dataclass_fields__) + ["states_history"]
    assert hip.FIELD_FRAME_STATE_NAMES == ("outside", "no_return", "in_front", "on", "behind")
    assert (hip.FIELD_FRAME_OUTSIDE, hip.FIELD_FRAME_NO_RETURN, hip.FIELD_FRAME_IN_FRONT, hip.FIELD_FRAME_ON, hip.FIELD_FRAME_BEHIND) == \
        (R.OUTSIDE, R.NO_RETURN, R.IN_FRONT, R.ON, R.BEHIND) == (0, 1, 2, 3, 4)


def _bad_frame_views():
    """``_bad_views`` without the two fields of the z-buffer, which a frame match does not read."""
    return [(p, v) for p, v in _bad_views() if not p.startswith(("footprint", "tolerance"))]


def _bad_searches(go, name, two={}):
    """Every way the arguments of the window search can be wrong, through ``go(**keywords)``; ``two`` makes it two problems."""
    for bad in (-0.1, float("nan"), float("inf"), 1e39, None, True, "0.4"):
        with pytest.raises(ValueError, match=name + ": max_distance must be a finite number >= 0"):
            go(max_distance=bad)
    for bad in (-1, 9, 4.0, True, None, "4"):
        with pytest.raises(ValueError, match=name + ": reach must be an integer in \\[0, 8\\]"):
            go(reach=bad)
    for bad in (-1e-3, float("nan"), float("inf"), None, False, "0.02"):
        with pytest.raises(ValueError, match=name + ": tolerance must be a finite number >= 0"):
            go(tolerance=bad)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match=name + ": keep_hidden must be a bool"):
            go(keep_hidden=bad)
    for bad in (None, _camera(), dict(height=48)):
        with pytest.raises(ValueError, match=name + ": the view must be a FieldView"):
            go(view=bad)
    for pattern, bad in _bad_frame_views():
        with pytest.raises(ValueError, match=name + ": " + pattern):
            go(view=bad, **two)
    frame = torch.zeros(48 * 64, 3)
    for bad in (None, frame.double(), frame[:, :2], frame[0], frame[:0], frame.numpy(), torch.zeros(2, 2, 48 * 64, 3)):
        with pytest.raises(ValueError, match=name + ": frame must be fp32 \\[T, 3\\] or \\[Mo, T, 3\\] with T >= 1"):
            go(frame=bad)
    for bad in (frame[:-1], torch.zeros(2, 48 * 32, 3)):
        with pytest.raises(ValueError, match=name + ": frame must hold V \\* height \\* width = 3072 rows"):
            go(frame=bad)
    with pytest.raises(ValueError, match=name + ": frame must hold V \\* height \\* width = 12 rows \\(got 3072\\)"):
        go(view=_view(height=3, width=4))


def test_frame_matches_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import frame_matches
    pts, frame = torch.zeros(2, 40, 3), torch.zeros(48 * 64, 3)

    def go(points=pts, frame=frame, view=DEFAULT, max_distance=0.4, **kw):
        return frame_matches(points, frame, _view() if view is DEFAULT else view, max_distance, **kw)

    for bad in (None, pts.double(), pts[..., :2], pts[0, 0], np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="frame_matches: points must be fp32 \\[n, 3\\] or \\[Mq, n, 3\\]"):
            go(points=bad)
    _bad_searches(go, "frame_matches")
    for points, cloud in ((torch.zeros(0, 40, 3), frame), (torch.zeros(65536, 1, 3), frame)):
        with pytest.raises(ValueError, match="frame_matches: 1 to 65535 problems"):
            go(points=points, frame=cloud)
    for points, cloud in ((pts, frame.expand(3, -1, -1)), (torch.zeros(3, 40, 3), frame.expand(2, -1, -1))):
        with pytest.raises(ValueError, match="frame_matches: frame and points hold one set or one per problem"):
            go(points=points, frame=cloud)
    with pytest.raises(ValueError, match="frame_matches: M \\* V \\* n must stay below 2\\*\\*31"):
        go(points=torch.zeros(1, 3).expand(2 ** 15, 2 ** 16, 3), frame=torch.zeros(1, 3), view=_view(height=1, width=1))
    for bad in (3, torch.ones(2, dtype=torch.int32), torch.ones(1)):
        with pytest.raises(ValueError, match="frame_matches: count must be one int32"):
            go(count=bad)
    for bad in (torch.zeros(40), torch.zeros(39, dtype=torch.int32), [0] * 40):
        with pytest.raises(ValueError, match="frame_matches: labels must be int32 \\[40\\]"):
            go(labels=bad)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="frame_matches: intrinsics must live on the device of points"):
            go(points=pts.cuda())
        view = _view()
        view.intrinsics, view.cam2world = view.intrinsics.cuda(), view.cam2world.cuda()
        with pytest.raises(ValueError, match="frame_matches: frame must live on the device of points"):
            go(points=pts.cuda(), view=view)
        with pytest.raises(ValueError, match="frame_matches: labels must live on the device of points"):
            go(points=pts.cuda(), frame=frame.cuda(), view=view, labels=torch.zeros(40, dtype=torch.int32))
    # the two fields of the z-buffer are not read: a view that visible_rows refuses is fine here
    for args, kw in (((pts, frame), {}), ((pts[0], frame[None]), dict(view=_view(footprint=9, tolerance=-1.0, near=0.5))),
                     ((pts, frame.expand(2, -1, -1)), dict(reach=0, tolerance=0.0, keep_hidden=True, max_distance=0.0,
                                                         count=torch.ones(1, dtype=torch.int32), labels=torch.zeros(40, dtype=torch.int32)))):
        with pytest.raises(ValueError, match="frame_matches: .*no CPU path"):
            go(*args, **kw)


def test_the_registrations_to_a_frame_check_their_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud, cloud_registration_frame, register_commands_frame
    tw, joints, tree, xyz, labels, _ = _cpu_arguments()
    chain = J.chain()
    n = xyz.shape[0]
    frame = torch.zeros(48 * 64, 3)
    info = torch.zeros(48 * 64, 6)
    cloud = FieldPointCloud(grid=FieldGrid(chain["origin"], chain["step"], chain["dims"]), index=torch.from_numpy(chain["index"]),
                            xyz=xyz, density=torch.ones(n), color=None, jacobian=None, count=torch.tensor([n], dtype=torch.int32))

    def forms(extra):
        def plain(frame=frame, max_distance=0.4, view=DEFAULT, **kw):
            return register_commands_frame(tw, xyz, labels, frame, max_distance, _view() if view is DEFAULT else view, **kw, **extra)

        def on_cloud(frame=frame, max_distance=0.4, view=DEFAULT, **kw):
            return cloud_registration_frame(cloud, labels, tw, frame, max_distance, _view() if view is DEFAULT else view, **kw, **extra)
        return (("register_commands_frame", plain), ("cloud_registration_frame", on_cloud))

    for extra in ({}, dict(observed_information=info)):
        for name, go in forms(extra):
            two = dict(frame=frame.expand(2, -1, -1)) if not extra else dict(init=torch.zeros(2, 3))
            _bad_searches(go, name, two)
            for pattern, view in _bad_views():                                  # the self-cull reads the whole view
                with pytest.raises(ValueError, match=name + ": " + pattern):
                    go(view=view, **two)
            with pytest.raises(ValueError, match=name + ": reg must be"):       # register_commands' own checks, under this name
                go(reg=-1.0)
            with pytest.raises(ValueError, match=name + ": rounds must be an integer"):
                go(rounds=0)
            with pytest.raises(ValueError, match=name + ": frame and points hold one set or one per problem"):
                go(frame=frame.expand(2, -1, -1), init=torch.zeros(3, 3))
            for kw in ({}, dict(reach=0, tolerance=0.5, keep_hidden=True, view=_view(footprint=0, tolerance=0.5, near=0.25)),
                       dict(frame=frame.expand(2, -1, -1), init=torch.zeros(2, 3))):
                if "observed_information" in extra and kw.get("frame") is not None:
                    continue
                with pytest.raises(ValueError, match=name + ": .*no CPU path"):
                    go(**kw)
    for bad in (info[:, :5], info[:-1], info.double(), torch.zeros(2, 48 * 64, 6), "info"):
        with pytest.raises(ValueError, match="register_commands_frame: observed_information must be fp32 \\[3072, 6\\] or \\[1, 3072, 6\\]"):
            register_commands_frame(tw, xyz, labels, frame, 0.4, _view(), observed_information=bad)
    with pytest.raises(ValueError, match="cloud_registration_frame: observed_information must be fp32"):
        cloud_registration_frame(cloud, labels, tw, frame, 0.4, _view(), observed_information=info[:, :5])
    with pytest.raises(ValueError, match="cloud_registration_frame: cloud must be a FieldPointCloud"):
        cloud_registration_frame(None, labels, tw, frame, 0.4, _view())
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="register_commands_frame: intrinsics must live on the device of xyz"):
            register_commands_frame(tw, xyz.cuda(), labels.cuda(), frame.cuda(), 0.4, _view())


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    assert "njf_field_frame" in declared and "njf_field_frame" in hip.EXPORTED_SYMBOLS and hasattr(lib, "njf_field_frame")
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    params = re.search(r"njf_field_frame\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_frame.argtypes) == ARGUMENTS
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_FRAME_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_FRAME_MATCH"] == hip.FIELD_FRAME_MATCH == 1
    assert defines["NJF_FIELD_FRAME_KEEP_HIDDEN"] == hip.FIELD_FRAME_KEEP_HIDDEN == 2
    assert "NJF_FIELD_FRAME_WAVE" not in header and not hasattr(hip, "FIELD_FRAME_WAVE")     # built, measured, deleted
    assert defines["NJF_FIELD_FRAME_MAX_REACH"] == hip.FIELD_FRAME_MAX_REACH == R.MAX_REACH == 8
    assert defines["NJF_FIELD_FRAME_STATES"] == hip.FIELD_FRAME_STATES == R.STATES == 5
    assert [defines[f"NJF_FIELD_FRAME_{n.upper()}"] for n in hip.FIELD_FRAME_STATE_NAMES] == [0, 1, 2, 3, 4]


def test_the_entry_refuses_bad_arguments_without_a_gpu(lib):
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("points", "count", "labels", "num_queries", "n", "num_problems", "frame", "num_frames", "k", "w2c", "views", "height", "width",
             "reach", "near", "tolerance", "max_distance", "pixel", "z", "state", "index", "distance2", "matched", "found", "states", "phases")

    def call(**kw):
        args = {k: P for k in names}
        args.update(num_queries=3, n=-1, num_problems=3, num_frames=3, views=2, height=48, width=64, reach=4, near=0.0, tolerance=0.02,
                    max_distance=0.4, phases=1)
        args.update(kw)
        return lib.njf_field_frame(*[args[k] for k in names], None)

    # every call that could pass its other checks keeps n = -1, so that none reaches a launch
    assert call() == E_SHAPE
    for key in ("points", "frame", "k", "w2c", "pixel", "z", "state", "index", "distance2", "matched", "found", "states"):
        assert call(**{key: None}) == E_NULL, key
        assert call(**{key: None}, phases=0) == E_NULL, key                          # a missing pointer is judged first
    assert call(count=None, labels=None) == E_SHAPE                                  # the two optional inputs
    for phases in (1, 3):
        assert call(phases=phases) == E_SHAPE
    for key, values in (("phases", (0, -1, 2, 4, 5, 6, 7, 8, 9, 16)), ("num_problems", (0, -1, 65536)), ("num_queries", (0, 2, 4, -3)),
                        ("num_frames", (0, 2, 4, -3)), ("views", (0, -1, 33)), ("reach", (-1, 9, 100)),
                        ("near", (-1.0, float("nan"), float("inf"))), ("tolerance", (-1e-3, float("nan"), float("inf"))),
                        ("max_distance", (-0.1, float("nan"), float("inf"), 1e39))):
        for bad in values:
            assert call(**{key: bad}) == E_VALUE, (key, bad)                         # (judged before the shapes)
    assert call(num_queries=1, num_frames=1) == E_SHAPE                              # Mq = Mo = 1 is fine
    assert call(reach=0, max_distance=0.0, tolerance=0.0) == E_SHAPE and call(reach=8, views=32) == E_SHAPE
    for kw in (dict(height=0), dict(width=0), dict(height=-4), dict(height=2 ** 16, width=2 ** 15),
               dict(height=2 ** 14, width=2 ** 14, num_frames=3, views=3), dict(height=2 ** 15, width=2 ** 15, views=2, num_frames=1),
               dict(n=2 ** 29, num_problems=2, num_queries=2, num_frames=2), dict(n=2 ** 30, num_problems=1, num_queries=1, num_frames=1)):
        assert call(**{"n": 0, **kw}) == E_SHAPE, kw


# ---- the conditions of the GPU tests, on the CPU ----------------------------------------------------------------------------------------------
OCCLUDER = (slice(24, 48), slice(36, 60))        # rows 24 .. 47, columns 36 .. 59 of the depth image
PLATE = 0.15                                     # in front of the nearest depth inside the rectangle


def occluded(depth, k, c2w):
    """Section 22's depth image with a plate in front of the distal link, and the organised cloud of its back-projection under
    max_jump: (depth [1, H, W], frame [H W, 3] fp32 with NaN where a pixel gives no point, the body pixels the plate hides)."""
    inside = depth[0][OCCLUDER]
    plated = depth.copy()
    plated[0][OCCLUDER] = inside[inside > 0].min() - PLATE
    frame = S.pinhole_points(plated, k, c2w, "z")[0].astype(F32)
    frame[~S.depth_mask(plated, max_jump=MAX_JUMP).reshape(-1)] = np.nan
    return plated, frame, int((inside > 0).sum())


def restated_frame_registration(s, k, c2w, frame, reach=4, tolerance=0.02, keep_hidden=False, height=HEIGHT, width=WIDTH):
    history = []
    out = N.register(s["twists"], s["xyz"], s["labels"], frame, 4 * s["step"], s["parts"], s["joints"], s["tree"], rounds=ROUNDS,
                     iterations=3, search=R.route(k, c2w, height, width, 1, 0.01, reach=reach, tolerance=tolerance, keep_hidden=keep_hidden,
                                                  history=history))
    out["visible_history"] = np.stack([h[0] for h in history]).astype(np.int32)
    out["states_history"] = np.stack([h[1] for h in history]).astype(np.int32)
    return out


@pytest.fixture(scope="module")
def scene():
    return section_22_scene()


def _error(out, planted):
    return float(np.abs(out["fit"]["commands"] - planted).max())


def test_a_window_that_covers_the_displacement_gives_the_cell_list_routes_commands(scene):
    s, k, c2w, planted, depth, frame = scene
    assert s["xyz"].shape[0] == 878 and frame.shape == (HEIGHT * WIDTH, 3) and abs(4 * s["step"] - 0.4) < 1e-12
    cells = restated_registration(s, k, c2w, frame)                    # today's route: the cull, then the unordered point set
    got = {reach: restated_frame_registration(s, k, c2w, frame, reach=reach) for reach in (1, 2, 4, 8)}
    errors = {reach: _error(out, planted) for reach, out in got.items()}
    print("|u - planted| by reach:", {r: f"{e:.3e}" for r, e in errors.items()}, "found",
          {r: out["found_history"][:, 0].tolist() for r, out in got.items()})
    for reach in (4, 8):
        assert errors[reach] <= CONVERGED                              # the condition the GPU test relies on
        assert (got[reach]["found_history"] == 175).all() and abs(errors[reach] - 3.945e-2) < 5e-5      # the figures of the issue
        for f in ("commands_history", "cost_history", "found_history"):
            assert got[reach][f].tobytes() == cells[f].tobytes(), (reach, f)                           # in every bit
        assert got[reach]["matches"]["index"].tobytes() == cells["matches"]["index"].tobytes()
    assert errors[1] > 4 * CONVERGED                                   # the window must cover the displacement
    assert abs(errors[2] - 7.70e-2) < 5e-4 and abs(errors[1] - 2.18e-1) < 5e-3 and (got[1]["found_history"] == 161).all()
    assert errors[4] < errors[2] < errors[1]


def test_rows_behind_a_foreign_object_are_freed_by_the_frame(scene):
    s, k, c2w, planted, depth, _ = scene
    plated, frame, hidden = occluded(depth, k, c2w)
    assert hidden == 192 and int((depth[0] > 0).sum()) == 792 and int(np.isfinite(frame).all(axis=1).sum()) == 1021
    freed = {(reach, tol): restated_frame_registration(s, k, c2w, frame, reach=reach, tolerance=tol)
             for reach, tol in ((4, 0.01), (4, 0.02), (4, 0.05), (8, 0.01), (8, 0.05))}
    kept = restated_frame_registration(s, k, c2w, frame, keep_hidden=True)
    cells = restated_registration(s, k, c2w, frame)
    d_kept, d_cells = _error(kept, planted), _error(cells, planted)
    print("|u - planted| behind the plate:", {key: f"{_error(out, planted):.3e}" for key, out in freed.items()},
          f"keep_hidden {d_kept:.3e}, cell list with the cull {d_cells:.3e}; states of the last round",
          freed[(4, 0.01)]["states_history"][-1, 0].tolist())
    for key, out in freed.items():
        assert _error(out, planted) <= 2 * CONVERGED, key              # the condition the GPU test relies on
        assert abs(_error(out, planted) - 6.247e-2) < 5e-5, key        # the figure of the issue
        assert out["states_history"][-1, 0].tolist()[1:] == [28, 0, 117, 30], key
        assert out["commands_history"].tobytes() == freed[(4, 0.01)]["commands_history"].tobytes(), key
    assert d_kept > 4 * CONVERGED and d_cells > 4 * CONVERGED          # matched to the plate instead
    assert abs(d_kept - 5.658e-1) < 5e-4 and abs(d_cells - 5.582e-1) < 5e-4


COMMANDS = ((0.5, -0.3, 0.0), (-0.6, 0.4, 0.0), (1.0, 1.0, 0.0))


def test_the_planted_command_explains_the_frame_best(scene):
    s, k, c2w, planted, depth, frame = scene
    on, share = [], []
    for u in (planted[0], (0.0, 0.0, 0.0)) + COMMANDS:
        posed = F.posed_targets(s["twists"], np.float32([u]), s["xyz"], s["labels"], s["parts"], s["joints"], s["tree"])
        seen = V.visible(posed, k, c2w, HEIGHT, WIDTH, 1, 0.01)
        got = R.matches(seen["culled"], frame, k, c2w, HEIGHT, WIDTH, 0.4, reach=4, tolerance=0.05)
        assert got["states"][0].sum() == 878 and got["states"][0, 1:].sum() == seen["visible"][0]
        on.append(int(got["states"][0, R.ON]))
        share.append(float(R.explained(got["states"])[0]))
    print("ON rows", on, "explained", [f"{v:.3f}" for v in share])
    assert on == [167, 141, 107, 123, 95]                              # the figures of the issue
    assert all(share[0] > v for v in share[1:])                        # strictly the largest
