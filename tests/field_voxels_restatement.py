"""numpy restatement of njf_field_depth_points' validity rules and of njf_field_voxels (include/njf_hip.h),
written from the header's text: the depth mask, a float64 pinhole back-projection to judge the points by, and the integer
sums, kept cells, centroids and fills of the voxel reduction."""
import numpy as np

QUANTUM = 1048576        # NJF_FIELD_VOXELS_QUANTUM: 2^20 steps per cell
F32 = np.float32


# ---- depth frames ------------------------------------------------------------------------------------------------------------------------
def depth_valid(depth, near=0.0, far=np.inf):
    """VALID: finite and near < d <= far, compared in float."""
    d = np.asarray(depth, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > F32(near)) & (d <= F32(far))


def depth_mask(depth, near=0.0, far=np.inf, max_jump=None):
    """[B,H,W] bool: the pixels that give a point.  With max_jump a valid pixel is dropped when a 4-neighbour inside the image
    has a valid depth dn with fabsf(d - dn) > max_jump * fminf(d, dn), every operation in float."""
    d = np.asarray(depth, dtype=F32)
    valid = depth_valid(d, near, far)
    if max_jump is None:
        return valid
    keep = valid.copy()
    b, h, w = d.shape
    for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        for row in range(h):
            for col in range(w):
                r2, c2 = row + dr, col + dc
                if not (0 <= r2 < h and 0 <= c2 < w):
                    continue
                for i in range(b):
                    if valid[i, row, col] and valid[i, r2, c2]:
                        a, n = d[i, row, col], d[i, r2, c2]
                        if F32(abs(F32(a - n))) > F32(F32(max_jump) * min(a, n)):
                            keep[i, row, col] = False
    return keep


def pixel_centres(height, width):
    """[H*W,2] float64 (x, y) of the pixel centres, row-major: x = (col + 0.5) / W, y = (row + 0.5) / H."""
    row, col = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return np.stack([(col.reshape(-1) + 0.5) / width, (row.reshape(-1) + 0.5) / height], axis=-1)


def pinhole_points(depth, intrinsics, cam2world, kind):
    """[B,H*W,3] float64: the back-projection of every pixel by a plain pinhole model, whatever its validity.  kind "z": the
    camera-space point is K^-1 [x, y, 1] * depth; kind "ray": the unit vector along it times depth."""
    d = np.asarray(depth, dtype=np.float64)
    b, h, w = d.shape
    xy1 = np.concatenate([pixel_centres(h, w), np.ones((h * w, 1))], axis=-1)
    out = np.empty((b, h * w, 3))
    for i in range(b):
        cam = xy1 @ np.linalg.inv(np.asarray(intrinsics[i], dtype=np.float64)).T
        if kind == "ray":
            cam = cam / np.linalg.norm(cam, axis=-1, keepdims=True)
        else:
            assert kind == "z"
            cam = cam / cam[:, 2:3]
        c2w = np.asarray(cam2world[i], dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            out[i] = (cam * d[i].reshape(-1, 1)) @ c2w[:3, :3].T + c2w[:3, 3]
    return out


# ---- voxel centroids ---------------------------------------------------------------------------------------------------------------------
def cell_coordinates(points, origin, cell):
    """t_c = (p_c - origin_c) * inv_cell in float, inv_cell = 1.0f / cell."""
    inv_cell = F32(1.0) / F32(cell)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((np.asarray(points, dtype=F32) - np.asarray(origin, dtype=F32)).astype(F32) * inv_cell).astype(F32)


def classify(points, origin, cell, dims, count=None):
    """(valid [T], inside [T], cell index [T] int64 (of the inside points), q [T,3] int64) of one problem."""
    p = np.asarray(points, dtype=F32)
    t_rows = p.shape[0]
    valid = np.isfinite(p).all(axis=-1) & (np.arange(t_rows) < (t_rows if count is None else min(int(count), t_rows)))
    t = cell_coordinates(p, origin, cell)
    with np.errstate(invalid="ignore"):
        f = np.floor(t)
        inside = valid & ((f >= 0) & (f < np.asarray(dims, dtype=F32))).all(axis=-1)
        q = np.rint(((t - f).astype(F32) * F32(QUANTUM)).astype(F32))
    fi = np.where(inside[:, None], f, 0).astype(np.int64)
    index = (fi[:, 0] * dims[1] + fi[:, 1]) * dims[2] + fi[:, 2]
    return valid, inside, index, np.where(inside[:, None], q, 0).astype(np.int64)


def cell_sums(index, q):
    """(cells ascending [n], k [n], S [n,3] int64) of the inside points given by their cell index and q."""
    cells, inverse, k = np.unique(index, return_inverse=True, return_counts=True)
    sums = np.zeros((cells.shape[0], 3), dtype=np.int64)
    np.add.at(sums, inverse.reshape(-1), q)
    return cells, k.astype(np.int64), sums


def centroids(cells, k, sums, origin, cell, dims):
    """(float)(origin_c + (cell_index_c + S_c / (k * 2^20)) * cell) in double with exactly this association."""
    axis = np.stack([cells // (dims[1] * dims[2]), (cells // dims[2]) % dims[1], cells % dims[2]], axis=-1).astype(np.float64)
    per = k.astype(np.float64)[:, None] * float(QUANTUM)
    return (np.asarray(origin, dtype=F32).astype(np.float64) + (axis + sums.astype(np.float64) / per) * np.float64(F32(cell))).astype(F32)


def voxels(points, origin, cell, dims, count=None, min_points=1, capacity=None):
    """njf_field_voxels on points [M,T,3]: dict of points [M,cap,3] f32, weight, cell [M,cap] i32, sums [M,cap,3] i64, count and
    outside [M] i32, with the fills NaN / 0 / -1 / 0 from min(count, capacity) on."""
    p = np.asarray(points, dtype=F32)
    m, t_rows = p.shape[:2]
    dims = tuple(int(d) for d in dims)
    cap = min(t_rows, dims[0] * dims[1] * dims[2]) if capacity is None else int(capacity)
    out = dict(points=np.full((m, cap, 3), np.nan, dtype=F32), weight=np.zeros((m, cap), dtype=np.int32),
               cell=np.full((m, cap), -1, dtype=np.int32), sums=np.zeros((m, cap, 3), dtype=np.int64),
               count=np.zeros(m, dtype=np.int32), outside=np.zeros(m, dtype=np.int32))
    for i in range(m):
        valid, inside, index, q = classify(p[i], origin, cell, dims, None if count is None else count[i])
        out["outside"][i] = int((valid & ~inside).sum())
        cells, k, sums = cell_sums(index[inside], q[inside])
        keep = k >= min_points
        cells, k, sums = cells[keep], k[keep], sums[keep]
        out["count"][i] = cells.shape[0]
        n = min(cells.shape[0], cap)
        out["points"][i, :n] = centroids(cells, k, sums, origin, cell, dims)[:n]
        out["weight"][i, :n] = k[:n]
        out["cell"][i, :n] = cells[:n]
        out["sums"][i, :n] = sums[:n]
    return out


def mean_bound(centroid, t_abs_max, cell):
    """The header's error bound per axis against the float64 mean of the same points: cell * (2^-21 + 4 * 2^-24 * max(|t|, 1)) +
    2^-24 |centroid| -- the quantisation, the three fp32 roundings in t, the output rounding."""
    return float(cell) * (2.0 ** -21 + 4 * 2.0 ** -24 * np.maximum(t_abs_max, 1.0)) + 2.0 ** -24 * np.abs(centroid)
