"""One rule for reading a row, on the device: njf_field_nearest and njf_field_normals (a lane and a wave per
row), njf_field_visible, njf_field_frame and njf_field_tsdf_sample are given ONE posed cloud, and the rows each of them treats as
not read -- shown by its documented fill -- are the complement of ``field_visible_restatement.read_rows``; njf_field_normals takes
no labels, so the rule without them.

300 rows: the launches with a lane per row span two workgroups of 256, those with a wave per row 75.  count = 257, so exactly one
row of the second workgroup is read.  NaN, +inf and -inf coordinates and labels of -1 sit on rows 0, 63, 64, 255 and 256 (the ends
of a wave and of a workgroup) and behind the count.  Every row that IS read lies in front of the one 8 x 8 camera, inside the 4^3
grid, whose nodes all have a weight, and next to its own copy in the observed cloud: it is matched, seen in a pixel and KNOWN, so
a row is either filled or plainly read in every entry.

Run with -m gpu."""
import numpy as np
import pytest
import torch

import field_visible_restatement as V

pytestmark = pytest.mark.gpu

F32 = np.float32
N, COUNT, M = 300, 257, 2
HEIGHT = WIDTH = 8
NAN_BITS = 0x7fc00000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _t(dev, v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def _np(t):
    return t.cpu().numpy()


def _scene():
    """clean [n, 3] in |x|, |y| <= 0.3, 1 <= z <= 2; the posed rows [2, n, 3] with the planted coordinates; labels [n]"""
    rng = np.random.default_rng(28)
    clean = np.stack([rng.uniform(-0.3, 0.3, N), rng.uniform(-0.3, 0.3, N), rng.uniform(1.0, 2.0, N)], axis=1).astype(F32)
    rows = np.stack([clean, clean])
    for m, i, axis, bad in ((0, 0, 0, np.nan), (0, 63, 1, np.inf), (0, 64, 2, -np.inf), (0, 280, 0, np.nan),
                            (1, 1, 2, np.nan), (1, 256, 0, np.inf), (1, 191, 1, -np.inf), (1, 299, 2, np.inf)):
        rows[m, i, axis] = bad
    labels = (np.arange(N) % 5).astype(np.int32)
    labels[[100, 255, 290]] = -1
    return clean, rows, labels


def _filled(dev, fields, shapes):
    out = {f: torch.empty(shapes[f], dtype=dtype, device=dev) for f, dtype in fields}
    for t in out.values():
        t.view(torch.uint8).fill_(0x5a)
    return out


def _entries(dev, clean, points, labels):
    """{entry: (not read, read)}, each bool [M, n], from the outputs of every entry on ``points`` [Mq, n, 3]"""
    from neural_jacobian_field_amd import hip
    p, lab, count = _t(dev, points), _t(dev, labels), torch.tensor([COUNT], dtype=torch.int32, device=dev)
    observed = _t(dev, clean[None])
    cells = hip.make_field_grid((-1.0, -1.0, 0.0), (0.5, 0.5, 0.5), (4, 4, 5))
    got = {}
    for name, wave in (("nearest, a lane per row", 0), ("nearest, a wave per row", hip.FIELD_NEAREST_WAVE)):
        out = _filled(dev, (("index", torch.int32), ("distance2", torch.float32), ("matched", torch.float32), ("found", torch.int32)),
                      dict(index=(M, N), distance2=(M, N), matched=(M, N, 3), found=(M,)))
        hip.field_nearest(observed, p, cells, 0.25, out, M, count=count, labels=lab, phase=hip.FIELD_NEAREST_ALL | wave)
        index, d2, matched = _np(out["index"]), _np(out["distance2"]), _np(out["matched"]).view(np.int32)
        got[name] = ((index == -1) & np.isposinf(d2) & (matched == NAN_BITS).all(axis=2),
                     (index == np.arange(N)) & (d2 == 0) & (_np(out["matched"]) == clean[None]).all(axis=2))
        assert (_np(out["found"]) == got[name][1].sum(axis=1)).all(), name
    for name, wave in (("normals, a lane per row", 0), ("normals, a wave per row", hip.FIELD_NORMALS_WAVE)):
        out = _filled(dev, (("moments", torch.int64), ("normal", torch.float32), ("neighbours", torch.int32), ("variation", torch.float32)),
                      dict(moments=(M, N, 10), normal=(M, N, 3), neighbours=(M, N), variation=(M, N)))
        hip.field_normals(observed, p, cells, 0.25, out, M, count=count, phase=hip.FIELD_NORMALS_ALL | wave)
        moments, neighbours = _np(out["moments"]), _np(out["neighbours"])
        got[name] = ((moments == 0).all(axis=2) & (neighbours == 0) & np.isnan(_np(out["normal"])).all(axis=2),
                     (moments[..., 0] >= 1) & (neighbours == moments[..., 0]))
    k = _t(dev, np.array([[[0.5, 0.0, 0.5], [0.0, 0.5, 0.5], [0.0, 0.0, 1.0]]], F32))   # |x / z|, |y / z| <= 0.3: inside the image
    w2c = _t(dev, np.eye(4, dtype=F32)[None])
    out = _filled(dev, hip.FIELD_VISIBLE_OUTPUTS, dict(depth=(M, 1, HEIGHT, WIDTH), index=(M, 1, HEIGHT, WIDTH), covered=(M, 1), seen=(M, N),
                                                       culled=(M, N, 3), visible=(M,), pixel=(M, 1, N), z=(M, 1, N)))
    hip.field_visible(p, k, w2c, HEIGHT, WIDTH, out, M, count=count, labels=lab)
    pixel, z = _np(out["pixel"])[:, 0], _np(out["z"])[:, 0]
    got["visible"] = ((pixel == -1) & (z.view(np.int32) == NAN_BITS) & (_np(out["seen"]) == 0) & np.isnan(_np(out["culled"])).all(axis=2),
                      (pixel >= 0) & (z >= 1.0))
    # (a row that is read is splatted: the winners of the z-buffer are read rows)
    winners = _np(out["index"]).reshape(M, -1)
    assert all(got["visible"][1][m, winners[m][winners[m] >= 0]].all() for m in range(M)) and (_np(out["covered"]) > 0).all()
    out = _filled(dev, hip.FIELD_FRAME_OUTPUTS, dict(pixel=(M, 1, N), z=(M, 1, N), state=(M, 1, N), index=(M, N), distance2=(M, N),
                                                     matched=(M, N, 3), found=(M,), states=(M, hip.FIELD_FRAME_STATES)))
    frame = _t(dev, np.tile(np.array([0.0, 0.0, 1.5], F32), (1, HEIGHT * WIDTH, 1)))
    hip.field_frame(p, frame, k, w2c, HEIGHT, WIDTH, 4.0, out, M, count=count, labels=lab, reach=1,
                    phase=hip.FIELD_FRAME_MATCH | hip.FIELD_FRAME_KEEP_HIDDEN)   # (a row behind the frame is matched too)
    pixel, z, state, index = _np(out["pixel"])[:, 0], _np(out["z"])[:, 0], _np(out["state"])[:, 0], _np(out["index"])
    got["frame"] = ((pixel == -1) & (z.view(np.int32) == NAN_BITS) & (state == hip.FIELD_FRAME_OUTSIDE) & (index == -1) &
                    np.isposinf(_np(out["distance2"])) & (_np(out["matched"]).view(np.int32) == NAN_BITS).all(axis=2),
                    (pixel >= 0) & (z >= 1.0) & (state >= hip.FIELD_FRAME_IN_FRONT) & (index >= 0))
    assert (_np(out["states"])[:, hip.FIELD_FRAME_OUTSIDE] == got["frame"][0].sum(axis=1)).all()
    grid = hip.make_field_grid((-0.5, -0.5, 0.5), (0.4, 0.4, 0.8), (4, 4, 4))
    values, weight = torch.full((1, 64), 0.125, device=dev), torch.ones(1, 64, device=dev)
    out = _filled(dev, hip.FIELD_TSDF_SAMPLE_OUTPUTS, dict(state=(M, N), distance=(M, N), gradient=(M, N, 3), states=(M, hip.FIELD_TSDF_STATES)))
    hip.field_tsdf_sample(p, grid, values, weight, out, M, count=count, labels=lab)
    state, distance = _np(out["state"]), _np(out["distance"])
    got["tsdf_sample"] = ((state == hip.FIELD_TSDF_OUTSIDE) & (distance.view(np.int32) == NAN_BITS) & np.isnan(_np(out["gradient"])).all(axis=2),
                          (state == hip.FIELD_TSDF_KNOWN) & (distance == F32(0.125)))
    assert (_np(out["states"])[:, hip.FIELD_TSDF_OUTSIDE] == got["tsdf_sample"][0].sum(axis=1)).all()
    return got


@pytest.mark.parametrize("mq", (1, 2))
def test_every_entry_leaves_out_the_rows_that_read_rows_leaves_out(dev, mq):
    clean, rows, labels = _scene()
    points = rows[:mq]
    want = {True: np.broadcast_to(V.read_rows(points, COUNT, labels), (M, N)), False: np.broadcast_to(V.read_rows(points, COUNT), (M, N))}
    # the planted rows do what they were planted for: one read row in the second workgroup (none where row 256 is infinite)
    assert want[True][0, 256:].sum() == 1 and not want[True][0, [0, 63, 64, 100, 255, 257, 280]].any() and want[False][0, 255]
    assert mq == 1 or (want[True][1, 256:].sum() == 0 and want[True][1, [0, 63, 64]].all() and not want[True][1, [1, 191, 255]].any())
    got = _entries(dev, clean, points, labels)
    assert len(got) == 7
    for name, (unread, read) in got.items():
        rule = want[not name.startswith("normals")]
        assert (unread == ~rule).all(), (name, np.argwhere(unread == rule)[:8])
        assert (read == rule).all(), (name, np.argwhere(read != rule)[:8])
