"""numpy restatement of the match of posed rows to a depth frame by projection (field_volume.frame_matches /
register_commands_frame; njf_field_frame), written from the semantics in include/njf_hip.h -- test
infrastructure only.

Two parts, as in field_visible_restatement, so that exactness is asked only where it can hold.  The projection is that module's
``project``, the pinhole model in float64.  ``finish`` takes per-row pixels and fp32 depths AS GIVEN -- the device's own, in the GPU
tests -- with the fp32 world-to-camera matrices as given, and restates the state rule, the clipped window, the distance and the
tie rule exactly: from there on every byte is determined.  ``matches`` composes the two for one point set, and ``route`` is the
``search`` hook that puts the self-cull and the frame match into ``field_nearest_restatement.register``'s loop."""
import numpy as np

import field_mesh_restatement as G
import field_nearest_restatement as N
import field_visible_restatement as V

F32 = np.float32
MAX_REACH = 8
OUTSIDE, NO_RETURN, IN_FRONT, ON, BEHIND = range(5)
STATES = 5
OUT = ("pixel", "z", "state", "index", "distance2", "matched", "found", "states")


def camera_z(w2c, p):
    """fp32 [n]: fmaf(w[10], p.z, fmaf(w[9], p.y, fmaf(w[8], p.x, w[11]))) for one fp32 matrix w2c [4, 4] and points p [n, 3]."""
    w, p = np.asarray(w2c, F32), np.asarray(p, F32)
    with np.errstate(all="ignore"):
        return G.fma32(w[2, 2], p[:, 2], G.fma32(w[2, 1], p[:, 1], G.fma32(w[2, 0], p[:, 0], np.broadcast_to(w[2, 3], p.shape[:1]))))


def states_of(pixel, z, own, w2c, tolerance):
    """int32 [n]: the state of rows with own pixels ``pixel`` [n] (-1 = none) and depths ``z`` [n] fp32 against the frame's points
    at those pixels, ``own`` [n, 3] fp32 (anything where the row has no pixel)."""
    z = np.asarray(z, F32)
    has, returned = np.asarray(pixel) >= 0, np.isfinite(own).all(axis=1)
    zo = camera_z(w2c, own)
    with np.errstate(all="ignore"):
        slack = (F32(tolerance) * zo).astype(F32)
        in_front, behind = (zo - z).astype(F32) > slack, (z - zo).astype(F32) > slack
    return np.where(~has, OUTSIDE, np.where(~returned, NO_RETURN, np.where(in_front, IN_FRONT, np.where(behind, BEHIND, ON)))).astype(np.int32)


def window(row, col, height, width, reach):
    """The pixels (r, c) of the window of reach ``reach`` around (row, col), clipped to the image, in ascending r * W + c."""
    return [(r, c) for r in range(max(row - reach, 0), min(row + reach, height - 1) + 1)
            for c in range(max(col - reach, 0), min(col + reach, width - 1) + 1)]


def finish(points, frame, pixel, z, read, w2c, problems, height, width, max_distance, reach=4, tolerance=0.02, keep_hidden=False):
    """Every output of the entry from per-row pixels [Mq, V, n] and depths [Mq, V, n] fp32 as given, for the rows ``read`` [Mq, n],
    the frame [Mo, V H W, 3] and the fp32 matrices w2c [V, 4, 4]: dict of pixel, state [M, V, n] int32, z [M, V, n] fp32, index [M, n]
    int32, distance2 [M, n] fp32, matched [M, n, 3] fp32, found [M] int32 and states [M, 5] int32."""
    assert 0 <= reach <= MAX_REACH
    points, frame = N._three(points), N._three(frame)
    (mq, n), mo, views, m_all = points.shape[:2], frame.shape[0], pixel.shape[1], int(problems)
    hw = height * width
    assert frame.shape[1] == views * hw and mq in (1, m_all) and mo in (1, m_all)
    max_d2 = F32(max_distance) * F32(max_distance)
    out = dict(pixel=np.full((m_all, views, n), -1, np.int32), z=np.full((m_all, views, n), np.nan, F32),
               state=np.zeros((m_all, views, n), np.int32), states=np.zeros((m_all, STATES), np.int32), **N._empty(m_all, n))
    for m in range(m_all):
        q, cloud = 0 if mq == 1 else m, frame[0 if mo == 1 else m]
        best, best_j = np.full(n, np.inf, F32), np.full(n, -1, np.int64)
        for v in range(views):
            pix = np.where(read[q], pixel[q, v], -1).astype(np.int64)
            zz = np.where(read[q], np.asarray(z[q, v], F32), F32(np.nan)).astype(F32)
            state = states_of(pix, zz, cloud[v * hw + pix.clip(0)], w2c[v], tolerance)
            out["pixel"][m, v], out["z"][m, v], out["state"][m, v] = pix, zz, state
            out["states"][m] += np.bincount(state, minlength=STATES).astype(np.int32)
            searched = (state != OUTSIDE) & ((state != BEHIND) | bool(keep_hidden))
            row, col = pix.clip(0) // width, pix.clip(0) % width
            for dr in range(-reach, reach + 1):
                for dc in range(-reach, reach + 1):
                    r, c = row + dr, col + dc
                    rows = np.flatnonzero(searched & (r >= 0) & (r < height) & (c >= 0) & (c < width))
                    j = v * hw + r[rows] * width + c[rows]
                    p = cloud[j]
                    ok = np.isfinite(p).all(axis=1)
                    rows, j, p = rows[ok], j[ok], p[ok]
                    with np.errstate(over="ignore"):
                        dx, dy, dz = (points[q][rows, a] - p[:, a] for a in range(3))
                        d2 = ((dx * dx + dy * dy) + dz * dz).astype(F32)
                    take = (best_j[rows] < 0) | (d2 < best[rows]) | ((d2 == best[rows]) & (j < best_j[rows]))
                    best[rows[take]], best_j[rows[take]] = d2[take], j[take]
        rows = np.flatnonzero(best_j >= 0)
        N._accept(out, m, rows, best_j[rows].astype(np.int32), best[rows], cloud, max_d2)
    return out


def matches(points, frame, k, c2w, height, width, max_distance, reach=4, tolerance=0.02, near=0.0, keep_hidden=False, count=None,
            labels=None, problems=None):
    """The whole entry for points [Mq, n, 3] from the float64 projection, its z rounded to fp32, and the float64 inverse of c2w
    rounded to fp32."""
    points, frame = N._three(points), N._three(frame)
    pr = V.project(points, k, c2w, height, width, near)
    with np.errstate(over="ignore", invalid="ignore"):
        z32 = pr["z"].astype(F32)
    w2c = np.linalg.inv(np.asarray(c2w, np.float64)).astype(F32)
    m = max(points.shape[0], frame.shape[0]) if problems is None else problems
    return finish(points, frame, pr["pixel"], z32, V.read_rows(points, count, labels), w2c, m, height, width, max_distance, reach,
                  tolerance, keep_hidden)


def explained(states):
    """float64 [M]: ON / (ON + IN_FRONT + NO_RETURN), NaN when the denominator is 0."""
    s = np.asarray(states, np.float64).reshape(-1, STATES)
    with np.errstate(invalid="ignore"):
        return s[:, ON] / (s[:, ON] + s[:, IN_FRONT] + s[:, NO_RETURN])


def route(k, c2w, height, width, footprint=1, cull_tolerance=0.01, near=0.0, reach=4, tolerance=0.02, keep_hidden=False, history=None):
    """A ``search`` hook of ``field_nearest_restatement.register`` whose ``observed`` is the frame: the self-cull of
    ``field_visible_restatement.visible``, then the frame match on the culled rows.  ``history`` (a list) receives every round's
    (visible [M], states [M, 5])."""
    def hook(frame, posed, max_distance, observed_count, count, labels):
        assert observed_count is None
        seen = V.visible(posed, k, c2w, height, width, footprint, cull_tolerance, near, count, labels)
        out = matches(seen["culled"], frame, k, c2w, height, width, max_distance, reach, tolerance, near, keep_hidden, count, labels)
        if history is not None:
            history.append((seen["visible"].copy(), out["states"].copy()))
        return out
    return hook
