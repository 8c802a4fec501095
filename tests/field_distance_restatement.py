"""numpy restatement of the fusion of depth frames into a truncated signed distance and of its sampling at rows
(field_volume.fuse_depth / sample_distance; njf_field_tsdf / njf_field_tsdf_sample), written from the
semantics in include/njf_hip.h -- test infrastructure only.

Two parts, as in field_visible_restatement, so that exactness is asked only where it can hold.  The projection of the nodes is that
module's ``project``, the pinhole model in float64.  ``fuse`` takes per-node pixels and fp32 depths AS GIVEN -- the device's own, in
the GPU tests: ``visible_rows(grid.points(), view)`` -- and restates the contribution rule and the three update cases exactly;
``sample`` restates the cell, the state, the interpolant and its derivative exactly from the fp32 field as given.  From there on
every byte is determined.  ``fuse_depth`` composes projection and fusion for one grid."""
import numpy as np

import field_mesh_restatement as G
import field_visible_restatement as V

F32 = np.float32
NAN32 = F32(np.nan)
OUTSIDE, UNKNOWN, KNOWN = range(3)
STATES = 3
OUT = ("values", "weight", "known")
SAMPLE_OUT = ("state", "distance", "gradient", "states")


def num_nodes(dims):
    return int(dims[0]) * int(dims[1]) * int(dims[2])


def node_points(origin, step, dims):
    """fp32 [N, 3]: the coordinates of all nodes in linear order, fmaf((float)i_c, step[c], origin[c])."""
    index = np.stack(np.unravel_index(np.arange(num_nodes(dims)), dims), axis=-1)
    return G.node_coordinates(origin, step, index).astype(F32)


def fuse(pixel, z, depth, near, far, truncation, max_weight=np.inf, values_in=None, weight_in=None):
    """Every output of njf_field_tsdf from per-node own pixels ``pixel`` [V, N] (row * W + col, -1 = not inside) and camera depths
    ``z`` [V, N] fp32 as given, for the images ``depth`` [M, V, H, W] fp32 and the state ``values_in``, ``weight_in`` [M, N] (both
    or neither): dict of values, weight [M, N] fp32 and known [M] int32."""
    depth = np.asarray(depth, F32)
    pixel, z = np.asarray(pixel, np.int64), np.asarray(z, F32)
    (m_all, views), n = depth.shape[:2], pixel.shape[1]
    assert pixel.shape == z.shape == (views, n) and (values_in is None) == (weight_in is None)
    near, far, truncation, max_weight = F32(near), F32(far), F32(truncation), F32(max_weight)
    flat = depth.reshape(m_all, views, -1)
    out = dict(values=np.empty((m_all, n), F32), weight=np.empty((m_all, n), F32), known=np.zeros(m_all, np.int32))
    for m in range(m_all):
        total, c = np.zeros(n, F32), np.zeros(n, F32)
        for v in range(views):                               # ascending: the order of the float additions
            has = pixel[v] >= 0
            d = flat[m, v][np.where(has, pixel[v], 0)]
            with np.errstate(all="ignore"):
                s = (d - z[v]).astype(F32)
                ok = has & np.isfinite(d) & (d > near) & (d <= far) & (s >= -truncation)
                total = np.where(ok, (total + np.minimum(s, truncation)).astype(F32), total)
            c = np.where(ok, (c + F32(1.0)).astype(F32), c)
        w0 = np.zeros(n, F32) if weight_in is None else np.asarray(weight_in, F32)[m]
        d0 = np.full(n, NAN32) if values_in is None else np.asarray(values_in, F32)[m]
        with np.errstate(all="ignore"):
            grown = (G.fma32(w0, d0, total).astype(F32) / (w0 + c).astype(F32)).astype(F32)
            first = (total / c).astype(F32)
            values = np.where(c == 0, d0, np.where(w0 > 0, grown, first))
            weight = np.where(c == 0, w0, np.where(w0 > 0, np.minimum((w0 + c).astype(F32), max_weight), np.minimum(c, max_weight)))
            out["values"][m], out["weight"][m] = values, weight
            out["known"][m] = int((weight > 0).sum())
    return out


def fuse_depth(origin, step, dims, depth, k, c2w, near, far, truncation, max_weight=np.inf, values_in=None, weight_in=None):
    """The whole entry for one grid from the float64 projection of its nodes, its z rounded to fp32."""
    depth = np.asarray(depth, F32)
    pr = V.project(node_points(origin, step, dims), k, c2w, depth.shape[2], depth.shape[3], near)
    with np.errstate(over="ignore", invalid="ignore"):
        z32 = pr["z"][0].astype(F32)
    return fuse(pr["pixel"][0], z32, depth, near, far, truncation, max_weight, values_in, weight_in)


def lerp(u, w, f):
    """fp32 fmaf(f, w - u, u), w - u a float subtraction."""
    with np.errstate(all="ignore"):
        return G.fma32(f, (np.asarray(w, F32) - np.asarray(u, F32)).astype(F32), u).astype(F32)


def sample(points, origin, step, dims, values, weight, count=None, labels=None, problems=None):
    """Every output of njf_field_tsdf_sample for points [Mq, n, 3] in the field values, weight [Mf, N] fp32 as given: dict of state
    [M, n] int32, distance [M, n] fp32, gradient [M, n, 3] fp32 and states [M, 3] int32."""
    points = np.asarray(points, F32)
    points = points[None] if points.ndim == 2 else points
    values, weight = np.asarray(values, F32), np.asarray(weight, F32)
    (mq, n), mf = points.shape[:2], values.shape[0]
    m_all = max(mq, mf) if problems is None else int(problems)
    assert mq in (1, m_all) and mf in (1, m_all) and all(d >= 2 for d in dims) and all(F32(s) > 0 for s in step)
    origin, step = np.asarray(origin, F32), np.asarray(step, F32)
    read = V.read_rows(points, count, labels)
    ny, nz = int(dims[1]), int(dims[2])
    out = dict(state=np.zeros((m_all, n), np.int32), distance=np.full((m_all, n), NAN32), gradient=np.full((m_all, n, 3), NAN32),
               states=np.zeros((m_all, STATES), np.int32))
    for m in range(m_all):
        q, val, wgt = 0 if mq == 1 else m, values[0 if mf == 1 else m], weight[0 if mf == 1 else m]
        with np.errstate(all="ignore"):
            g = ((points[q] - origin[None]).astype(F32) / step[None]).astype(F32)                       # [n, 3]
            inside = read[q] & ((g >= 0) & (g <= (np.asarray(dims, np.int64) - 1).astype(F32)[None])).all(axis=1)
        rows = np.flatnonzero(inside)
        gi = g[rows]
        cell = np.minimum(np.floor(gi).astype(np.int64), np.asarray(dims, np.int64)[None] - 2)
        f = (gi - cell.astype(F32)).astype(F32)
        base = (cell[:, 0] * ny + cell[:, 1]) * nz + cell[:, 2]
        corner = lambda a, b, c: base + (a * ny + b) * nz + c                                           # noqa: E731
        known = np.ones(len(rows), bool)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    known &= ~(wgt[corner(a, b, c)] == 0)
        state = np.zeros(n, np.int32)
        state[rows] = np.where(known, KNOWN, UNKNOWN)
        rows, f = rows[known], f[known]
        C = [[[val[corner(a, b, c)[known]] for c in (0, 1)] for b in (0, 1)] for a in (0, 1)]
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        e = [[lerp(C[a][b][0], C[a][b][1], fz) for b in (0, 1)] for a in (0, 1)]
        h = [lerp(e[a][0], e[a][1], fy) for a in (0, 1)]
        with np.errstate(all="ignore"):
            qd = [(e[a][1] - e[a][0]).astype(F32) for a in (0, 1)]
            r = [[(C[a][b][1] - C[a][b][0]).astype(F32) for b in (0, 1)] for a in (0, 1)]
            t = [lerp(r[a][0], r[a][1], fy) for a in (0, 1)]
            out["distance"][m, rows] = lerp(h[0], h[1], fx)
            out["gradient"][m, rows, 0] = ((h[1] - h[0]).astype(F32) / step[0]).astype(F32)
            out["gradient"][m, rows, 1] = (lerp(qd[0], qd[1], fx) / step[1]).astype(F32)
            out["gradient"][m, rows, 2] = (lerp(t[0], t[1], fx) / step[2]).astype(F32)
        out["state"][m] = state
        out["states"][m] = np.bincount(state, minlength=STATES).astype(np.int32)
    return out


def cost(state, distance):
    """float64 [M]: the mean of |distance| over the KNOWN rows, NaN with none."""
    known = np.asarray(state) == KNOWN
    total = np.where(known, np.abs(np.asarray(distance, np.float64)), 0.0).sum(axis=1)
    with np.errstate(invalid="ignore"):
        return total / known.sum(axis=1).astype(np.float64)


def surface_targets(points, state, distance, gradient):
    """(targets [M, n, 3], normals [M, n, 3]) in float64: x - distance g / (g . g) and g / |g| for the KNOWN rows with g . g > 0, NaN
    for the others."""
    p, g = np.asarray(points, np.float64), np.asarray(gradient, np.float64)
    gg = (g * g).sum(axis=-1, keepdims=True)
    ok = (np.asarray(state) == KNOWN)[..., None] & (gg > 0)
    with np.errstate(all="ignore"):
        targets = np.where(ok, p - np.asarray(distance, np.float64)[..., None] * g / gg, np.nan)
        normals = np.where(ok, g / np.sqrt(gg), np.nan)
    return targets, normals
