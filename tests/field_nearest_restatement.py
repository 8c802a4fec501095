"""numpy restatement of the closest-point query and the registration loop (field_volume.nearest_points / register_commands;
njf_field_nearest), written from the semantics in include/njf_hip.h -- test infrastructure only.

``brute`` is the definition: for every searched query row the valid observed point of the smallest ``(dx*dx + dy*dy) + dz*dz`` in
fp32, ties to the lowest index, accepted within ``max_distance``.  ``rings`` restates the ALGORITHM -- the points sorted into
cells, Chebyshev rings around the query's cell, the stop rule -- and must give the same bytes.  ``register`` composes the loop
from the restatements of the pose (field_pose_restatement) and of the solver (field_commands_restatement)."""
import numpy as np

import field_commands_restatement as F

MAX_RINGS = 64
MAX_DIM = 1024
NAN32 = np.float32(np.nan)


def _three(a):
    a = np.asarray(a, dtype=np.float32)
    return a[None] if a.ndim == 2 else a


def _problems(observed, queries):
    mo, mq = observed.shape[0], queries.shape[0]
    m = max(mo, mq)
    assert mo in (1, m) and mq in (1, m)
    return m


def valid_points(observed, observed_count=None):
    """bool [Mo, T]: j < min(observed_count[m], T) and three finite coordinates."""
    observed = _three(observed)
    mo, t = observed.shape[:2]
    limit = np.full(mo, t) if observed_count is None else np.minimum(np.maximum(np.asarray(observed_count).reshape(mo), 0), t)
    return (np.arange(t)[None, :] < limit[:, None]) & np.isfinite(observed).all(axis=2)


def searched_rows(queries, count=None, labels=None):
    """bool [Mq, n]: i < min(count, n), three finite coordinates, label >= 0 when labels are given.  Rows from the count on
    are not READ: their coordinates play no part."""
    queries = _three(queries)
    n = queries.shape[1]
    rows = n if count is None else min(max(int(count), 0), n)
    ok = np.zeros(queries.shape[:2], bool)
    ok[:, :rows] = np.isfinite(queries[:, :rows]).all(axis=2)
    if labels is not None:
        ok &= (np.asarray(labels) >= 0)[None, :]
    return ok


def _empty(m, n):
    return dict(index=np.full((m, n), -1, np.int32), distance2=np.full((m, n), np.inf, np.float32),
                matched=np.full((m, n, 3), NAN32, np.float32), found=np.zeros(m, np.int32))


def _d2(q, p):
    """fp32 [rows, points]: (dx*dx + dy*dy) + dz*dz, every operation rounded to fp32."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
        return (dx * dx + dy * dy) + dz * dz


def _accept(out, i, rows, j, d2, points, max_d2):
    ok = d2 <= max_d2
    out["index"][i, rows[ok]] = j[ok]
    out["distance2"][i, rows[ok]] = d2[ok]
    out["matched"][i, rows[ok]] = points[j[ok]]
    out["found"][i] += int(ok.sum())


def brute(observed, queries, max_distance, observed_count=None, count=None, labels=None, chunk=256):
    """dict of index [M, n] int32, distance2 [M, n] fp32, matched [M, n, 3] fp32, found [M] int32 by the definition."""
    observed, queries = _three(observed), _three(queries)
    m, n = _problems(observed, queries), queries.shape[1]
    valid, rows_of = valid_points(observed, observed_count), searched_rows(queries, count, labels)
    max_d2 = np.float32(max_distance) * np.float32(max_distance)
    out = _empty(m, n)
    for i in range(m):
        pts, q = observed[0 if observed.shape[0] == 1 else i], queries[0 if queries.shape[0] == 1 else i]
        js = np.flatnonzero(valid[0 if observed.shape[0] == 1 else i])          # ascending: argmin's first hit is the lowest j
        rows = np.flatnonzero(rows_of[0 if queries.shape[0] == 1 else i])
        if not js.size:
            continue
        for lo in range(0, rows.size, chunk):
            part = rows[lo:lo + chunk]
            d2 = _d2(q[part], pts[js])
            best = d2.argmin(axis=1)
            _accept(out, i, part, js[best].astype(np.int32), d2[np.arange(part.size), best], pts, max_d2)
    return out


def cell_of(p, origin, cell, dims):
    """int [..., 3]: clamp(floor((p_c - origin_c) * (1 / cell)), 0, dims_c - 1) in fp32."""
    inv = np.float32(1.0) / np.float32(cell)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor((np.asarray(p, np.float32) - np.asarray(origin, np.float32)) * inv)
    return np.minimum(np.maximum(f, np.float32(0.0)), (np.asarray(dims) - 1).astype(np.float32)).astype(np.int64)


def check_lattice(origin, cell, dims, max_distance):
    assert all(1 <= d <= MAX_DIM for d in dims) and np.float32(cell) > 0 and np.float32(max_distance) > 0
    assert np.ceil(float(np.float32(max_distance)) / float(np.float32(cell))) + 1 <= MAX_RINGS


def rings(observed, queries, origin, cell, dims, max_distance, observed_count=None, count=None, labels=None):
    """The same dict as ``brute`` by the cell list and the ring search, with ``rings`` [M, n] (the last ring visited, -1 = not
    searched) and ``records`` [M, n] (the records read)."""
    observed, queries = _three(observed), _three(queries)
    check_lattice(origin, cell, dims, max_distance)
    m, n = _problems(observed, queries), queries.shape[1]
    valid, rows_of = valid_points(observed, observed_count), searched_rows(queries, count, labels)
    reach, cell = np.float32(max_distance), np.float32(cell)
    max_d2 = reach * reach
    dx, dy, dz = (int(d) for d in dims)
    out = _empty(m, n)
    out["rings"], out["records"] = np.full((m, n), -1, np.int32), np.zeros((m, n), np.int64)
    lists = {}
    for i in range(m):
        io, iq = (0 if observed.shape[0] == 1 else i), (0 if queries.shape[0] == 1 else i)
        pts, q = observed[io], queries[iq]
        if io not in lists:
            js = np.flatnonzero(valid[io])
            c = cell_of(pts[js], origin, cell, dims)
            linear = (c[:, 0] * dy + c[:, 1]) * dz + c[:, 2]
            order = np.argsort(linear, kind="stable")
            lists[io] = (js[order], np.searchsorted(linear[order], np.arange(dx * dy * dz + 1)))
        record, start = lists[io]
        rows = np.flatnonzero(rows_of[iq])
        qc = cell_of(q[rows], origin, cell, dims)
        for row, (cx, cy, cz) in zip(rows, qc):
            best, best_j, read, last = np.float32(np.inf), -1, 0, -1
            for r in range(MAX_RINGS + 1):                     # the centre cell and at most MAX_RINGS rings
                if r >= 2:                                     # rings 0 .. r - 1 are done: the rest is (r - 1) cells away or more
                    lim = (np.float32(r - 1) - np.float32(1.0 / 128.0)) * cell
                    if best < lim * lim or lim > reach:
                        break
                if cx - r < 0 and cx + r >= dx and cy - r < 0 and cy + r >= dy and cz - r < 0 and cz + r >= dz:
                    break                                      # no cell at this distance, nor at a larger one
                last = r
                spans = []
                for x in range(max(cx - r, 0), min(cx + r, dx - 1) + 1):
                    for y in range(max(cy - r, 0), min(cy + r, dy - 1) + 1):
                        column = (x * dy + y) * dz
                        if x in (cx - r, cx + r) or y in (cy - r, cy + r):
                            spans.append((column + max(cz - r, 0), column + min(cz + r, dz - 1)))
                        else:
                            spans += [(column + z, column + z) for z in (cz - r, cz + r) if 0 <= z < dz]
                cand = np.concatenate([record[start[c0]:start[c1 + 1]] for c0, c1 in spans]) if spans else np.zeros(0, np.int64)
                read += cand.size
                if cand.size:
                    d2 = _d2(q[row][None], pts[cand])[0]
                    pick = np.lexsort((cand, d2))[0]
                    if d2[pick] < best or (d2[pick] == best and cand[pick] < best_j) or best_j < 0:
                        best, best_j = d2[pick], int(cand[pick])
            out["rings"][i, row], out["records"][i, row] = last, read
            if best_j >= 0 and best <= max_d2:
                out["index"][i, row], out["distance2"][i, row], out["matched"][i, row] = best_j, best, pts[best_j]
                out["found"][i] += 1
    return out


def register(twists, xyz, labels, observed, max_distance, parts, joints=None, tree=None, observed_count=None, count=None,
             weights=None, init=None, lower=None, upper=None, reg=0.0, rounds=8, iterations=3, damping=1e-3, search=brute):
    """The registration loop: dict of ``fit`` and ``matches`` (the last round's), commands_history [R, M, A] fp32, cost_history
    [R, M] float64, found_history [R, M] int32.  ``search(observed, queries, max_distance, observed_count, count, labels)``."""
    observed = _three(observed)
    a_dim = np.asarray(twists["omega"]).shape[1]
    m = max(observed.shape[0], 1 if init is None else np.asarray(init).shape[0])
    box = lambda v, fill: np.broadcast_to(np.asarray(fill if v is None else v, dtype=np.float32), (m, a_dim))   # noqa: E731
    u = np.minimum(np.maximum(box(init, 0.0), box(lower, -np.inf)), box(upper, np.inf)).astype(np.float32)
    out = dict(commands_history=np.zeros((rounds, m, a_dim), np.float32), cost_history=np.zeros((rounds, m)),
               found_history=np.zeros((rounds, m), np.int32))
    for r in range(rounds):
        posed = F.posed_targets(twists, u, xyz, labels, parts, joints, tree, count=count)
        near = search(observed, posed, max_distance, observed_count, count, labels)
        fit = F.solve(twists, xyz, labels, near["matched"], parts, joints, tree, weights=weights, count=count, init=u, lower=lower,
                      upper=upper, reg=reg, iterations=iterations, damping=damping)
        out["commands_history"][r], out["cost_history"][r], out["found_history"][r] = fit["commands"], fit["cost"], near["found"]
        out["fit"], out["matches"], u = fit, near, fit["commands"]
    return out
