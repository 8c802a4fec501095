"""numpy restatement of the z-buffer of posed rows (field_volume.visible_rows / FieldView; njf_field_visible; DESIGN.md section
24), written from the semantics in include/njf_hip.h -- test infrastructure only.

Three parts, so that exactness is asked only where it can hold.  ``project`` is the pinhole model in float64: the device's fp32
projection is held to it within a bound, and to its pixel wherever the row is not on a pixel edge.  ``rasterise`` and
``test_rows`` take per-row pixels and fp32 depths AS GIVEN -- the device's own, in the GPU tests -- and restate the key rule and
the tolerance rule exactly: from there on every byte is determined.  ``visible`` composes the three for one point set, and
``cull`` is the ``search`` hook that puts it in front of ``field_nearest_restatement.register``'s closest-point query."""
import numpy as np

import field_nearest_restatement as N

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_VIEWS, MAX_FOOTPRINT = 32, 4


def read_rows(points, count=None, labels=None):
    """bool [Mq, n]: i < min(count, n), three finite coordinates, label >= 0 when labels are given (nearest's searched row)."""
    return N.searched_rows(points, count, labels)


def project(points, k, c2w, height, width, near=0.0):
    """The pinhole model in float64 for points [Mq, n, 3] (or [n, 3]) through the cameras k [V, 3, 3] (normalised intrinsics) and
    c2w [V, 4, 4]: dict of z [Mq, V, n] float64 (the camera-space z), x and y [Mq, V, n] float64 (the continuous pixel
    coordinates u * W and v * H), col and row (their floors, int64; 0 where not finite), projectable (z finite and > near),
    inside (projectable, 0 <= col < W, 0 <= row < H) and pixel [Mq, V, n] int64 (row * W + col, -1 where not inside)."""
    p = np.asarray(points, np.float64)
    p = p[None] if p.ndim == 2 else p
    k, c2w = np.asarray(k, np.float64), np.asarray(c2w, np.float64)
    w2c = np.linalg.inv(c2w)
    with np.errstate(all="ignore"):
        cam = np.einsum("vab,mnb->mvna", w2c[:, :3, :3], p) + w2c[:, None, :3, 3][None]
        z = cam[..., 2]
        s, t = cam[..., 0] / z, cam[..., 1] / z
        x = (k[:, 0, 0, None] * s + k[:, 0, 1, None] * t + k[:, 0, 2, None]) * width
        y = (k[:, 1, 0, None] * s + k[:, 1, 1, None] * t + k[:, 1, 2, None]) * height
        projectable = np.isfinite(z) & (z > float(F32(near)))
        fx, fy = np.floor(x), np.floor(y)
        inside = projectable & (fx >= 0) & (fx < width) & (fy >= 0) & (fy < height)
    finite = np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 2 ** 40) & (np.abs(fy) < 2 ** 40)
    col, row = np.where(finite, fx, 0).astype(np.int64), np.where(finite, fy, 0).astype(np.int64)
    return dict(z=z, x=x, y=y, col=col, row=row, projectable=projectable, inside=inside, pixel=np.where(inside, row * width + col, -1))


def keys_of(z, rows=None):
    """uint64 [n]: (bits(z) << 32) | row for fp32 z."""
    z = np.ascontiguousarray(z, F32)
    rows = np.arange(z.shape[0]) if rows is None else np.asarray(rows)
    return (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)


def rasterise(pixel, z, n, height, width, footprint, outside=None):
    """One image from the per-row own pixels ``pixel`` [n] (row * W + col, -1 = the row has none) and depths ``z`` [n] fp32, by the
    key rule: every row with a pixel writes (bits(z) << 32) | i, as a uint64 minimum, into the pixels within ``footprint`` of its
    own that lie in the image.  ``outside``: int [j, 3] of (i, row, col) for the projectable rows whose own pixel lies outside
    the image (their ``pixel`` is -1) -- their footprint may still reach in.  (depth [H, W] fp32 -- 0 = empty --, index [H, W]
    int32 -- -1 = empty --, covered)."""
    pixel, z = np.asarray(pixel, np.int64).reshape(n), np.asarray(z, F32).reshape(n)
    rows = np.flatnonzero(pixel >= 0)
    row, col = pixel[rows] // width, pixel[rows] % width
    if outside is not None and len(outside):
        outside = np.asarray(outside, np.int64).reshape(-1, 3)
        assert (pixel[outside[:, 0]] < 0).all()
        rows, row, col = np.concatenate([rows, outside[:, 0]]), np.concatenate([row, outside[:, 1]]), np.concatenate([col, outside[:, 2]])
    key = keys_of(z[rows], rows)
    image = np.full(height * width, EMPTY, np.uint64)
    for dr in range(-footprint, footprint + 1):
        for dc in range(-footprint, footprint + 1):
            r, c = row + dr, col + dc
            ok = (r >= 0) & (r < height) & (c >= 0) & (c < width)
            np.minimum.at(image, r[ok] * width + c[ok], key[ok])
    won = image != EMPTY
    depth = np.where(won, (image >> np.uint64(32)).astype(np.uint32).view(F32), F32(0.0)).astype(F32)
    index = np.where(won, (image & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth.reshape(height, width), index.reshape(height, width), int(won.sum())


def test_rows(pixel, z, depth, tolerance):
    """bool [n]: the row has an own pixel and z - zmin <= tolerance * zmin there, a float subtraction, a float product and a
    comparison, zmin = depth at the own pixel."""
    pixel, z = np.asarray(pixel, np.int64), np.asarray(z, F32)
    has = pixel >= 0
    zmin = np.asarray(depth, F32).reshape(-1)[np.where(has, pixel, 0)]
    with np.errstate(invalid="ignore"):
        return has & ((z - zmin).astype(F32) <= (F32(tolerance) * zmin).astype(F32))


test_rows.__test__ = False      # (a restatement, not a test: the name is the issue's)


def outside_rows(pr, m, v, footprint, height, width):
    """``rasterise``'s ``outside`` for problem m and view v of a ``project`` result: the projectable rows whose own pixel lies
    outside the image but within ``footprint`` of it."""
    near_by = pr["projectable"][m, v] & ~pr["inside"][m, v] & (pr["col"][m, v] >= -footprint) & (pr["col"][m, v] < width + footprint) \
        & (pr["row"][m, v] >= -footprint) & (pr["row"][m, v] < height + footprint)
    rows = np.flatnonzero(near_by)
    return np.stack([rows, pr["row"][m, v][rows], pr["col"][m, v][rows]], axis=1)


def finish(points, pixel, z, read, outside, problems, height, width, footprint, tolerance):
    """Every output of the entry from per-row pixels [Mq, V, n] and depths [Mq, V, n] fp32 as given: dict of depth, index [M, V, H,
    W], covered [M, V], seen [M, n] int32, culled [M, n, 3] fp32, visible [M] int32, pixel [M, V, n] int32 and z [M, V, n] fp32
    (-1 and NaN on the rows that are not ``read`` [Mq, n]).  ``outside(m, v)`` gives ``rasterise``'s list."""
    points = np.asarray(points, F32)
    points = points[None] if points.ndim == 2 else points
    mq, n = points.shape[:2]
    views, m_all = pixel.shape[1], int(problems)
    out = dict(depth=np.zeros((m_all, views, height, width), F32), index=np.full((m_all, views, height, width), -1, np.int32),
               covered=np.zeros((m_all, views), np.int32), seen=np.zeros((m_all, n), np.int32),
               culled=np.full((m_all, n, 3), np.nan, F32), visible=np.zeros(m_all, np.int32),
               pixel=np.full((m_all, views, n), -1, np.int32), z=np.full((m_all, views, n), np.nan, F32))
    for m in range(m_all):
        q = 0 if mq == 1 else m
        for v in range(views):
            pix = np.where(read[q], pixel[q, v], -1)
            zz = np.where(read[q], np.asarray(z[q, v], F32), F32(np.nan)).astype(F32)
            extra = outside(q, v)
            extra = extra[read[q][extra[:, 0]]] if len(extra) else extra
            out["depth"][m, v], out["index"][m, v], out["covered"][m, v] = rasterise(pix, zz, n, height, width, footprint, extra)
            out["seen"][m] |= test_rows(pix, zz, out["depth"][m, v], tolerance).astype(np.int32) << v
            out["pixel"][m, v], out["z"][m, v] = pix, zz
        hit = out["seen"][m] != 0
        out["culled"][m][hit] = points[q][hit]
        out["visible"][m] = int(hit.sum())
    return out


def visible(points, k, c2w, height, width, footprint=1, tolerance=0.01, near=0.0, count=None, labels=None, problems=None):
    """The whole entry for points [Mq, n, 3] from the float64 projection, its z rounded to fp32."""
    points = np.asarray(points, F32)
    points = points[None] if points.ndim == 2 else points
    pr = project(points, k, c2w, height, width, near)
    read = read_rows(points, count, labels)
    with np.errstate(over="ignore", invalid="ignore"):
        z32 = pr["z"].astype(F32)
    return finish(points, pr["pixel"], z32, read, lambda m, v: outside_rows(pr, m, v, footprint, height, width),
                  points.shape[0] if problems is None else problems, height, width, footprint, tolerance)


def cull(k, c2w, height, width, footprint=1, tolerance=0.01, near=0.0, search=N.brute, history=None):
    """A ``search`` hook of ``field_nearest_restatement.register``: the closest-point query on the rows the cameras see, the
    others NaN (not searched).  ``history`` (a list) receives every round's visible counts [M]."""
    def hook(observed, posed, max_distance, observed_count, count, labels):
        seen = visible(posed, k, c2w, height, width, footprint, tolerance, near, count, labels)
        if history is not None:
            history.append(seen["visible"].copy())
        return search(observed, seen["culled"], max_distance, observed_count, count, labels)
    return hook
