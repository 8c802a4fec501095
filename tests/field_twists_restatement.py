"""Numpy float64 restatement of the rigid-twist fit (field_volume.fit_twists; njf_field_twists in include/njf_hip.h; DESIGN.md
section 15), written from the stated semantics:

* rows ``xyz [n, 3]``, ``jacobian [n, A, 3]`` fp32, ``labels [n]`` int32, optional ``weights [n]`` fp32 with
  ``w = weights > 0 ? weights : 0`` (NaN and negatives: 0), a row count, a part list ``parts [K]`` and the true ``parts_count``;
  row i belongs to slot p iff ``i < count``, ``p < min(parts_count, K)`` and ``labels[i] == parts[p]``; a row of weight 0 counts
  in ``nodes`` and enters no sum;
* pass A: ``W = sum w``, ``S = sum w*x``, ``c = S / W``;  pass B with ``r = x - c``: ``Q = sum w*(r_a*r_b)`` (xx, xy, xz, yy, yz,
  zz), per channel ``P = sum w*J``, ``L = sum w*(r x J)``, ``E = sum w*((Jx*Jx + Jy*Jy) + Jz*Jz)``;
* solve: ``M = tr(Q) I - Q``, Cholesky in the order x, y, z, a pivot ``<= 1e-9 tr(M)`` makes the part translation-only (status
  bit 2, ``omega = 0``), else ``omega = M^-1 L``; ``v = P / W``; ``W == 0``: status bit 1 and a zero slot;
* pass C: ``residual = sum w*|J - (v + omega x r)|^2`` and the unweighted ``row_residual = sum_a |J_a - model|^2`` in fp32.

Every TERM is formed in float64 with the operations in the order written (numpy's element-wise arithmetic is IEEE, one rounding
per operation, no contraction), so the terms are bit for bit the ones the kernels add; every SUM is ``math.fsum`` (correctly
rounded), so the only difference to the device is its summation order.  ``fit`` also returns, per raw sum, the sum of the
absolute terms and the number of terms: what the first-order bound of a reordered sum needs.  ``fit_loop`` is the same fit
written node by node in Python floats, against which the vectorised form is itself checked."""
import math

import numpy as np

EMPTY, TRANSLATION = 1, 2
PIVOT_FLOOR = 1e-9
U = 2.0 ** -53


def effective_weights(weights, n):
    if weights is None:
        return np.ones(n, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, w, np.float32(0)).astype(np.float64)


def _fsum(terms):
    return math.fsum(terms.tolist())


def _cross(a, b):
    """a x b along the last axis, each component as (a1*b2 - a2*b1)."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def solve(q, l_rows):
    """(omega [A, 3], full) from Q (6) and L [A, 3]: Cholesky of M = tr(Q) I - Q in the order x, y, z."""
    q = [float(v) for v in q]
    tr = (q[0] + q[3]) + q[5]
    mxx, myy, mzz, mxy, mxz, myz = tr - q[0], tr - q[3], tr - q[5], -q[1], -q[2], -q[4]
    floor = PIVOT_FLOOR * ((mxx + myy) + mzz)
    zero = np.zeros((len(l_rows), 3))
    if not mxx > floor:
        return zero, False
    l11 = math.sqrt(mxx)
    l21, l31 = mxy / l11, mxz / l11
    d2 = myy - l21 * l21
    if not d2 > floor:
        return zero, False
    l22 = math.sqrt(d2)
    l32 = (myz - l31 * l21) / l22
    d3 = mzz - (l31 * l31 + l32 * l32)
    if not d3 > floor:
        return zero, False
    l33 = math.sqrt(d3)
    om = np.zeros((len(l_rows), 3))
    for a, l in enumerate(l_rows):
        y0 = float(l[0]) / l11
        y1 = (float(l[1]) - l21 * y0) / l22
        y2 = (float(l[2]) - (l31 * y0 + l32 * y1)) / l33
        w2 = y2 / l33
        w1 = (y1 - l32 * w2) / l22
        w0 = (y0 - (l21 * w1 + l31 * w2)) / l11
        om[a] = (w0, w1, w2)
    return om, True


def m_matrix(q):
    tr = (q[0] + q[3]) + q[5]
    return np.array([[tr - q[0], -q[1], -q[2]], [-q[1], tr - q[3], -q[4]], [-q[2], -q[4], tr - q[5]]], dtype=np.float64)


def fit(xyz, jacobian, labels, parts, parts_count=None, count=None, weights=None, centroid=None):
    """The fit as a dict of numpy arrays named like FieldTwists' fields, plus ``abs`` (per raw sum W, S, Q, P, L, E: the sum of
    the absolute terms) and ``terms`` [K] (rows of positive weight: the number of terms of every sum).  ``centroid`` [K, 3]:
    form pass B and C around these centroids instead of the fit's own (the sums are defined relative to the centroid)."""
    xyz = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    jac = np.asarray(jacobian, dtype=np.float32).astype(np.float64)
    labels = np.asarray(labels)
    parts = np.asarray(parts)
    n, a_dim, k = xyz.shape[0], jac.shape[1], parts.shape[0]
    rows = n if count is None else min(max(int(count), 0), n)
    true_parts = k if parts_count is None else max(int(parts_count), 0)
    active = min(true_parts, k)
    w_all = effective_weights(weights, n)
    out = dict(labels=np.full(k, -1, np.int32), count=np.array([true_parts], np.int32), nodes=np.zeros(k, np.int32),
               status=np.zeros(k, np.int32), weight=np.zeros(k), centroid=np.zeros((k, 3)), omega=np.zeros((k, a_dim, 3)),
               velocity=np.zeros((k, a_dim, 3)), energy=np.zeros((k, a_dim)), residual=np.zeros((k, a_dim)), Q=np.zeros((k, 6)),
               P=np.zeros((k, a_dim, 3)), L=np.zeros((k, a_dim, 3)), row_residual=np.zeros(n, np.float32), terms=np.zeros(k, np.int64))
    absolute = dict(W=np.zeros(k), S=np.zeros((k, 3)), Q=np.zeros((k, 6)), P=np.zeros((k, a_dim, 3)), L=np.zeros((k, a_dim, 3)),
                    E=np.zeros((k, a_dim)))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for p in range(active):
        member = np.flatnonzero(labels[:rows] == parts[p])
        out["labels"][p] = parts[p]
        out["nodes"][p] = member.size
        used = member[w_all[member] > 0]
        out["terms"][p] = used.size
        w, x, j = w_all[used], xyz[used], jac[used]
        big_w = _fsum(w)
        absolute["W"][p] = big_w
        c = np.zeros(3)
        if big_w > 0:
            for d in range(3):
                t = w * x[:, d]
                c[d] = _fsum(t) / big_w
                absolute["S"][p, d] = _fsum(np.abs(t))
            out["weight"][p] = big_w
        else:
            out["status"][p] = EMPTY
        out["centroid"][p] = c
        if centroid is not None:
            c = np.asarray(centroid, dtype=np.float64)[p]
        r = x - c
        for e, (d0, d1) in enumerate(pairs):
            t = w * (r[:, d0] * r[:, d1])
            out["Q"][p, e], absolute["Q"][p, e] = _fsum(t), _fsum(np.abs(t))
        for a in range(a_dim):
            ja = j[:, a, :]
            rxj = _cross(r, ja)
            for d in range(3):
                t = w * ja[:, d]
                out["P"][p, a, d], absolute["P"][p, a, d] = _fsum(t), _fsum(np.abs(t))
                t = w * rxj[:, d]
                out["L"][p, a, d], absolute["L"][p, a, d] = _fsum(t), _fsum(np.abs(t))
            t = w * ((ja[:, 0] * ja[:, 0] + ja[:, 1] * ja[:, 1]) + ja[:, 2] * ja[:, 2])
            out["energy"][p, a] = absolute["E"][p, a] = _fsum(t)
        if big_w > 0:
            out["velocity"][p] = out["P"][p] / big_w
            om, full = solve(out["Q"][p], out["L"][p])
            out["omega"][p] = om
            if not full:
                out["status"][p] |= TRANSLATION
        # pass C on every row of the part (the row residual is unweighted: rows of weight 0 get one too)
        with np.errstate(invalid="ignore", over="ignore"):
            r_all = xyz[member] - c
            row = np.zeros(member.size)
            for a in range(a_dim):
                model = out["velocity"][p, a] + _cross(np.broadcast_to(out["omega"][p, a], r_all.shape), r_all)
                d = jac[member, a, :] - model
                t = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                row = row + t
                keep = w_all[member] > 0
                out["residual"][p, a] = _fsum(w_all[member][keep] * t[keep]) if big_w > 0 else 0.0
            out["row_residual"][member] = row.astype(np.float32)
    out["abs"] = absolute
    return out


def fit_loop(xyz, jacobian, labels, parts, parts_count=None, count=None, weights=None):
    """The same fit, node by node in Python floats (which are IEEE doubles): (nodes, weight, centroid, Q, P, L, energy, omega,
    velocity, residual, status) per slot, with the terms collected in lists and summed by ``math.fsum``."""
    xyz = np.asarray(xyz, dtype=np.float32)
    jac = np.asarray(jacobian, dtype=np.float32)
    n, a_dim, k = xyz.shape[0], jac.shape[1], len(parts)
    rows = n if count is None else min(max(int(count), 0), n)
    active = min(k if parts_count is None else max(int(parts_count), 0), k)
    slots = []
    for p in range(k):
        if p >= active:
            slots.append(None)
            continue
        member = []
        for i in range(rows):
            if int(labels[i]) != int(parts[p]):
                continue
            w = 1.0 if weights is None else float(weights[i])
            member.append((i, w if w > 0 else 0.0))
        used = [(i, w) for i, w in member if w > 0]
        big_w = math.fsum(w for _, w in used)
        c = [math.fsum(w * float(xyz[i, d]) for i, w in used) / big_w if big_w > 0 else 0.0 for d in range(3)]
        r = {i: [float(xyz[i, d]) - c[d] for d in range(3)] for i, _ in used}
        q = [math.fsum(w * (r[i][d0] * r[i][d1]) for i, w in used) for d0, d1 in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        big_p, big_l, energy = np.zeros((a_dim, 3)), np.zeros((a_dim, 3)), np.zeros(a_dim)
        for a in range(a_dim):
            jf = {i: [float(jac[i, a, d]) for d in range(3)] for i, _ in used}
            for d in range(3):
                d1, d2 = (d + 1) % 3, (d + 2) % 3
                big_p[a, d] = math.fsum(w * jf[i][d] for i, w in used)
                big_l[a, d] = math.fsum(w * (r[i][d1] * jf[i][d2] - r[i][d2] * jf[i][d1]) for i, w in used)
            energy[a] = math.fsum(w * ((jf[i][0] * jf[i][0] + jf[i][1] * jf[i][1]) + jf[i][2] * jf[i][2]) for i, w in used)
        status, om, vel, residual = 0, np.zeros((a_dim, 3)), np.zeros((a_dim, 3)), np.zeros(a_dim)
        if big_w > 0:
            vel = big_p / big_w
            om, full = solve(q, big_l)
            status = 0 if full else TRANSLATION
            for a in range(a_dim):
                terms = []
                for i, w in used:
                    o, v, ri = om[a], vel[a], r[i]
                    model = [v[0] + (o[1] * ri[2] - o[2] * ri[1]), v[1] + (o[2] * ri[0] - o[0] * ri[2]), v[2] + (o[0] * ri[1] - o[1] * ri[0])]
                    d = [float(jac[i, a, e]) - model[e] for e in range(3)]
                    terms.append(w * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
                residual[a] = math.fsum(terms)
        else:
            status = EMPTY
        slots.append(dict(nodes=len(member), weight=big_w, centroid=np.array(c), Q=np.array(q), P=big_p, L=big_l, energy=energy,
                          omega=om, velocity=vel, residual=residual, status=status))
    return slots


def lstsq_twist(xyz, jacobian_a, w, centre):
    """(omega, v at ``centre``) of one channel by ``np.linalg.lstsq`` on the 6-unknown system sqrt(w) (v + omega x (x - centre)) =
    sqrt(w) J: the definition the centred normal equations are checked against."""
    r = np.asarray(xyz, dtype=np.float64) - centre
    m = r.shape[0]
    a = np.zeros((m, 3, 6))
    a[:, 0, 0] = a[:, 1, 1] = a[:, 2, 2] = 1.0
    # omega x r = -[r]x omega
    a[:, 0, 4], a[:, 0, 5] = r[:, 2], -r[:, 1]
    a[:, 1, 3], a[:, 1, 5] = -r[:, 2], r[:, 0]
    a[:, 2, 3], a[:, 2, 4] = r[:, 1], -r[:, 0]
    s = np.sqrt(np.asarray(w, dtype=np.float64))[:, None, None]
    sol = np.linalg.lstsq((a * s).reshape(3 * m, 6), (np.asarray(jacobian_a, dtype=np.float64) * s[:, :, 0]).reshape(3 * m), rcond=None)[0]
    return sol[3:], sol[:3]


# ---- the shared fixture: boxes of grid nodes, one label per box ---------------------------------------------------------------
DIMS = (17, 19, 23)
LOWER, UPPER = (-0.97, -0.91, 0.83), (1.03, 0.87, 2.05)
# (element, ix0, nx, iy0, ny, iz0, nz) or a list of nodes; in the order of the issue
BOXES = (("one node", 0, [(1, 1, 1)]),
         ("collinear", 0, [(3, 3, 3), (4, 4, 4), (5, 5, 5)]),
         ("2x2x2", 0, (7, 2, 1, 2, 1, 2)),
         ("one layer", 0, (10, 1, 2, 5, 3, 6)),
         ("12x9x7", 0, (2, 12, 9, 9, 12, 7)),
         ("16x17x18", 1, (0, 16, 1, 17, 2, 18)))
DEGENERATE = ("one node", "collinear")
PAD = 37


def node_points(index):
    """fp32 coordinates of global node indices: fma(i, step, origin) per axis, the grid's definition."""
    n_nodes = DIMS[0] * DIMS[1] * DIMS[2]
    node = np.asarray(index, dtype=np.int64) % n_nodes
    yz = DIMS[1] * DIMS[2]
    comps = (node // yz, (node % yz) // DIMS[2], node % DIMS[2])
    cols = []
    for i, lo, hi, d in zip(comps, LOWER, UPPER, DIMS):
        step = np.float32((float(hi) - float(lo)) / (d - 1))
        cols.append((i.astype(np.float64) * np.float64(step) + np.float64(np.float32(lo))).astype(np.float32))
    return np.stack(cols, axis=-1)


def fixture(seed=0, unlabelled=300):
    """Rows in ascending global index: the nodes of BOXES (label = the box's smallest global index, so the labels of the
    second element exceed N), ``unlabelled`` other nodes with label -1 between them, and PAD rows past ``count`` that repeat a
    fitted label with NaN coordinates (they must never be read).  Returns a dict: index, xyz, labels [n + PAD], count, parts
    (ascending), names (per part)."""
    rng = np.random.default_rng(seed)
    n_nodes = DIMS[0] * DIMS[1] * DIMS[2]
    label_of = {}
    names = {}
    for name, element, spec in BOXES:
        if isinstance(spec, list):
            cells = spec
        else:
            x0, nx, y0, ny, z0, nz = spec
            cells = [(x, y, z) for x in range(x0, x0 + nx) for y in range(y0, y0 + ny) for z in range(z0, z0 + nz)]
        g = sorted(element * n_nodes + (x * DIMS[1] + y) * DIMS[2] + z for x, y, z in cells)
        assert not set(g) & set(label_of), name
        for i in g:
            label_of[i] = g[0]
        names[g[0]] = name
    free = np.setdiff1d(np.arange(2 * n_nodes), np.fromiter(label_of, dtype=np.int64))
    for i in rng.choice(free, size=unlabelled, replace=False):
        label_of[int(i)] = -1
    index = np.array(sorted(label_of), dtype=np.int64)
    labels = np.array([label_of[int(i)] for i in index], dtype=np.int32)
    parts = np.array(sorted(names), dtype=np.int32)
    count = index.size
    xyz = node_points(index)
    # the padding: rows a fit that ignored the count would add to the largest part
    index = np.concatenate([index, np.full(PAD, index[-1])])
    labels = np.concatenate([labels, np.full(PAD, parts[-1], dtype=np.int32)])
    xyz = np.concatenate([xyz, np.full((PAD, 3), np.nan, dtype=np.float32)])
    return dict(index=index.astype(np.int32), xyz=xyz, labels=labels, count=count, parts=parts,
                names=[names[int(p)] for p in parts])


def planted_field(xyz, labels, parts, a_dim, seed):
    """A rigid field per part: J = fp32(v + omega x (x - q)) with twists rounded to fp32 first.  Returns (jacobian [n, A, 3]
    fp32, omega [K, A, 3], v [K, A, 3], q [K, 3]) -- the planted values as float64 of their fp32 roundings."""
    rng = np.random.default_rng(seed)
    k, n = len(parts), xyz.shape[0]
    omega = rng.normal(size=(k, a_dim, 3)).astype(np.float32).astype(np.float64)
    vel = rng.normal(size=(k, a_dim, 3)).astype(np.float32).astype(np.float64)
    q = rng.uniform(-0.5, 0.5, size=(k, 3)).astype(np.float32).astype(np.float64)
    jac = rng.normal(size=(n, a_dim, 3)).astype(np.float32)           # rows of no part keep noise
    x = xyz.astype(np.float64)
    for p, label in enumerate(parts):
        rows = np.flatnonzero(labels == label)
        with np.errstate(invalid="ignore"):
            r = x[rows] - q[p]
            for a in range(a_dim):
                jac[rows, a, :] = (vel[p, a] + _cross(np.broadcast_to(omega[p, a], r.shape), r)).astype(np.float32)
    return jac, omega, vel, q


def fixture_weights(fx, seed, zeros=0.0):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, size=fx["labels"].shape[0]).astype(np.float32)
    if zeros:
        w[rng.random(w.shape[0]) < zeros] = 0.0
    return w


def extent(ref, p):
    return math.sqrt(((ref["Q"][p, 0] + ref["Q"][p, 3]) + ref["Q"][p, 5]) / ref["weight"][p])


def planted_error(fx, a_dim=3, seed=11):
    """max over the non-degenerate parts and channels of the restatement's error against the planted twist, relative to
    max(|omega| * extent, |v at the centroid|), in velocity units (an omega error times the extent).  The planted Jacobians are
    rounded to fp32 (2^-24 relative per component), which is all that separates the fit from the plant."""
    jac, omega, vel, q = planted_field(fx["xyz"], fx["labels"], fx["parts"], a_dim, seed)
    w = fixture_weights(fx, seed + 1)
    ref = fit(fx["xyz"], jac, fx["labels"], fx["parts"], count=fx["count"], weights=w)
    worst = 0.0
    for p, name in enumerate(fx["names"]):
        if name in DEGENERATE:
            continue
        ext = extent(ref, p)
        v_at_c = vel[p] + _cross(omega[p], np.broadcast_to(ref["centroid"][p] - q[p], omega[p].shape))
        for a in range(a_dim):
            scale = max(np.linalg.norm(omega[p, a]) * ext, np.linalg.norm(v_at_c[a]))
            worst = max(worst, np.linalg.norm(ref["omega"][p, a] - omega[p, a]) * ext / scale,
                        np.linalg.norm(ref["velocity"][p, a] - v_at_c[a]) / scale)
    return worst, (jac, omega, vel, q, w, ref)
