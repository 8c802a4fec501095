"""numpy restatement of the normals of an observed cloud (field_volume.point_normals; njf_field_normals),
written from the semantics in include/njf_hip.h -- test infrastructure only.

``brute_moments`` is the definition of the neighbourhood and of the ten integer sums, by brute force over all points;
``ring_moments`` restates the cells visited (the Chebyshev rings 0 .. R) and must give the same integers.  ``finish`` turns
the sums into normals with ``numpy.linalg.eigh`` -- the judge of the device's Jacobi rotations, not a copy of them -- and
applies the sign rules.  ``float_pca`` is the un-quantised float64 covariance, against which the quantisation is measured."""
import numpy as np

import field_nearest_restatement as N

MOMENTS = 10
SCALE = 262144.0        # 2^18
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # [xx xy xz yy yz zz]
NAN32 = np.float32(np.nan)


def ring_count(cell, radius):
    """R: the smallest r >= 1 with ((float)r - 1/128) * cell > (float)radius, in fp32."""
    cell, reach = np.float32(cell), np.float32(radius)
    r = 1
    while r < N.MAX_RINGS and not (np.float32(r) - np.float32(1.0 / 128.0)) * cell > reach:
        r += 1
    return r


def offsets(q, pts):
    """fp32 [P, 3]: e = p - q, every difference rounded to fp32."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (pts - q[None, :]).astype(np.float32)


def within(e, radius):
    """bool [P]: (ex*ex + ey*ey) + ez*ez <= (float)radius * (float)radius in fp32."""
    r2 = np.float32(radius) * np.float32(radius)
    with np.errstate(over="ignore", invalid="ignore"):
        return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] <= r2


def quantise(e, radius):
    """int64 [P, 3]: k = rint((double)e * scale), scale = 2^18 / (double)(float)radius; ties to even."""
    scale = SCALE / float(np.float32(radius))
    return np.rint(e.astype(np.float64) * scale).astype(np.int64)


def sums(k):
    """int64 [10]: S0, S1[3], S2[6] of the quantised offsets ``k`` [P, 3] (python integers inside: no overflow to hide)."""
    out = [int(k.shape[0])] + [int(k[:, c].sum()) for c in range(3)]
    out += [int((k[:, a] * k[:, b]).sum()) for a, b in PAIRS]
    return np.array(out, dtype=np.int64)


def _sets(observed, queries):
    observed, queries = N._three(observed), N._three(queries)
    return observed, queries, N._problems(observed, queries)


def brute_moments(observed, queries, radius, observed_count=None, count=None):
    """int64 [M, n, 10] by the definition: every valid point against every searched row."""
    observed, queries, m = _sets(observed, queries)
    n = queries.shape[1]
    valid, rows_of = N.valid_points(observed, observed_count), N.searched_rows(queries, count)
    out = np.zeros((m, n, MOMENTS), np.int64)
    for i in range(m):
        io, iq = (0 if observed.shape[0] == 1 else i), (0 if queries.shape[0] == 1 else i)
        pts = observed[io][valid[io]]
        for row in np.flatnonzero(rows_of[iq]):
            e = offsets(queries[iq, row], pts)
            out[i, row] = sums(quantise(e[within(e, radius)], radius))
    return out


def ring_moments(observed, queries, origin, cell, dims, radius, observed_count=None, count=None):
    """(int64 [M, n, 10], records read [M, n]) by the cell list: the cells of the Chebyshev rings 0 .. R around the row's own
    cell, clipped to the lattice."""
    observed, queries, m = _sets(observed, queries)
    N.check_lattice(origin, cell, dims, radius)
    n = queries.shape[1]
    valid, rows_of = N.valid_points(observed, observed_count), N.searched_rows(queries, count)
    reach = ring_count(cell, radius)
    out, read = np.zeros((m, n, MOMENTS), np.int64), np.zeros((m, n), np.int64)
    for i in range(m):
        io, iq = (0 if observed.shape[0] == 1 else i), (0 if queries.shape[0] == 1 else i)
        pts = observed[io][valid[io]]
        cells = N.cell_of(pts, origin, cell, dims)
        rows = np.flatnonzero(rows_of[iq])
        for row, c in zip(rows, N.cell_of(queries[iq, rows], origin, cell, dims)):
            near = pts[(np.abs(cells - c[None, :]).max(axis=1) <= reach)] if pts.shape[0] else pts
            e = offsets(queries[iq, row], near)
            out[i, row], read[i, row] = sums(quantise(e[within(e, radius)], radius)), near.shape[0]
    return out, read


def covariance(moments):
    """float64 [..., 3, 3] and the counts: C_ab = S2_ab / N - mean_a mean_b (NaN where N = 0)."""
    s = np.asarray(moments)
    count = s[..., 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s[..., 1:4] / count[..., None]
        c = np.empty(s.shape[:-1] + (3, 3))
        for e, (a, b) in enumerate(PAIRS):
            c[..., a, b] = c[..., b, a] = s[..., 4 + e] / count - mean[..., a] * mean[..., b]
    return c, s[..., 0]


def orient(normal, queries, viewpoint=None):
    """(the normals [..., 3] float64 under the sign rule, the deciding quantity [...]): with a finite viewpoint n . (v - q) /
    |v - q| must not be negative; without, the component of largest magnitude (ties to the lowest axis) is positive, and the
    deciding quantity is the smaller of that magnitude and its lead over the runner-up's."""
    normal = np.array(normal, dtype=np.float64)
    mags = np.abs(normal)
    axis = mags.argmax(axis=-1)                                   # the first of equals: the lowest axis
    big = np.take_along_axis(normal, axis[..., None], -1)[..., 0]
    ordered = np.sort(mags, axis=-1)
    decide = np.where(big < 0, -1.0, 1.0)
    margin = np.minimum(ordered[..., 2], ordered[..., 2] - ordered[..., 1])
    if viewpoint is not None:
        v = np.broadcast_to(np.asarray(viewpoint, np.float32).astype(np.float64).reshape(-1, 1, 3), normal.shape)
        seen = np.isfinite(v).all(axis=-1)
        with np.errstate(invalid="ignore", over="ignore"):
            d = v - np.asarray(queries, np.float32).astype(np.float64)
            toward = (normal[..., 0] * d[..., 0] + normal[..., 1] * d[..., 1]) + normal[..., 2] * d[..., 2]
            length = np.sqrt((d * d).sum(axis=-1))
        decide = np.where(seen, np.where(toward < 0, -1.0, 1.0), decide)
        margin = np.where(seen, np.abs(toward) / np.where(length > 0, length, 1.0), margin)
    return normal * decide[..., None], margin


def finish(moments, queries, radius, min_neighbours=3, viewpoint=None, count=None):
    """dict of normal [M, n, 3] fp32, neighbours [M, n] int32, variation [M, n] fp32, eigenvalues [M, n, 3] float64 (NaN where
    there is no normal) and, for the tests, ``normal64`` (before the fp32 rounding), ``lam`` (the clamped eigenvalues in k^2
    units, ascending), ``has`` (rows with a normal) and ``margin`` (the deciding quantity of the sign rule).  Rows from the
    count on are not read."""
    moments = np.asarray(moments, dtype=np.int64)
    m, n = moments.shape[:2]
    queries = np.broadcast_to(N._three(queries), (m, n, 3))
    rows = n if count is None else min(max(int(count), 0), n)
    live = np.zeros((m, n), bool)
    live[:, :rows] = True
    c, s0 = covariance(np.where(live[..., None], moments, 0))
    enough = live & (s0 >= min_neighbours)
    lam, vec = np.linalg.eigh(np.where(enough[..., None, None], c, np.eye(3)))
    lam = np.maximum(lam, 0.0)
    total = (lam[..., 0] + lam[..., 1]) + lam[..., 2]
    has = enough & (total > 0)
    normal64, margin = orient(vec[..., :, 0], queries, viewpoint)
    scale = SCALE / float(np.float32(radius))
    nan = np.full((m, n), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        variation = np.where(has, lam[..., 0] / total, nan)
    normal64 = np.where(has[..., None], normal64, np.nan)
    return dict(normal=normal64.astype(np.float32), neighbours=np.where(live, s0, 0).astype(np.int32),
                variation=variation.astype(np.float32), eigenvalues=np.where(has[..., None], lam / (scale * scale), np.nan),
                normal64=normal64, lam=lam, has=has, margin=np.where(has, margin, nan))


def normals(observed, queries, radius, observed_count=None, count=None, min_neighbours=3, viewpoint=None):
    """``finish`` of ``brute_moments``, with ``moments``."""
    moments = brute_moments(observed, queries, radius, observed_count, count)
    if viewpoint is not None and moments.shape[0] == 1:            # Mo = Mq = 1: one problem per viewpoint
        moments = np.broadcast_to(moments, (np.asarray(viewpoint).reshape(-1, 3).shape[0],) + moments.shape[1:])
    out = finish(moments, queries, radius, min_neighbours, viewpoint, count)
    out["moments"] = moments
    return out


def float_pca(observed, queries, radius):
    """float64 [n, 3]: the eigenvector of the smallest eigenvalue of the UN-quantised covariance of the neighbours' offsets
    (one cloud, one set of rows; NaN below three neighbours), and the eigenvalues [n, 3]."""
    observed, queries = np.asarray(observed, np.float32), np.asarray(queries, np.float32)
    pts = observed[np.isfinite(observed).all(axis=1)]
    out, lams = np.full(queries.shape, np.nan), np.full(queries.shape, np.nan)
    for row in np.flatnonzero(np.isfinite(queries).all(axis=1)):
        e = offsets(queries[row], pts)
        e = e[within(e, radius)].astype(np.float64)
        if e.shape[0] >= 3:
            d = e - e.mean(axis=0)
            lam, vec = np.linalg.eigh(d.T @ d / e.shape[0])
            out[row], lams[row] = vec[:, 0], lam
    return out, lams


def sines(a, b):
    """|sin| of the angle between the directions ``a`` and ``b`` [..., 3] (float64; the sign of either plays no part)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        cross = np.cross(a, b)
        return np.sqrt((cross * cross).sum(axis=-1)) / (np.sqrt((a * a).sum(axis=-1)) * np.sqrt((b * b).sum(axis=-1)))


def torus(n, seed, noise=0.0, major=0.5, minor=0.2):
    """(points [n, 3] fp32, true unit normals [n, 3] float64) of a torus around the z axis sampled uniformly in its two angles,
    plus isotropic Gaussian noise."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    normal = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    centre = np.stack([major * np.cos(u), major * np.sin(u), np.zeros(n)], axis=1)
    return (centre + minor * normal + noise * rng.standard_normal((n, 3))).astype(np.float32), normal
