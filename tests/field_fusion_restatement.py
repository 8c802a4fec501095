"""Numpy restatement of the multi-view fusion semantics, written from the text, not from the kernels.

Batch layout: the B context images are G = B / V scenes of V consecutive views, batch element b = g*V + v.  ``s_v`` is the
frustum predicate of view v (all ones without cameras), ``c`` the number of views that see a node; a node is valid iff
``c >= min_views``.

* ``fuse``: the fused density of every node in float32 with the stated operation order --
  "mean": acc = 0; for v ascending: if s_v: acc += d_v; fused = acc / float(c);
  "min" / "max": start from the first seen view, then m = (d_v < m) ? d_v : m (``>`` for "max") over the later seen views;
  an invalid node has fused = 0.
* ``combine``: the attributes at a position in float64 -- w_v = s_v ? d_v : 0, W = sum of the w_v by float32 adds with v
  ascending, all w_v = 1 and W = V if not W > 0, out = (sum_v w_v x_v) / W.  The weights and W are the float32 numbers the
  device uses; only the weighted sum and the division are carried out in float64.
* ``combine_bound``: 2 * (2V + 2) * 2**-24 * max_v |x_v| per element: the first-order rounding bound of the V-term fma chain,
  the weight sum and one division, doubled for the higher-order terms."""
import numpy as np

MODES = ("mean", "min", "max")


def fuse(values, seen, mode, min_views):
    """values [G, V, N] float32, seen [G, V, N] bool -> (fused [G, N] float32, seen bitmask [G, N] uint8, valid [G, N] bool)."""
    values = np.asarray(values, dtype=np.float32)
    seen = np.asarray(seen, dtype=bool)
    assert values.shape == seen.shape and values.ndim == 3 and mode in MODES
    g, v, n = values.shape
    assert 1 <= min_views <= v <= 8
    count = np.zeros((g, n), dtype=np.int32)
    mask = np.zeros((g, n), dtype=np.uint8)
    acc = np.zeros((g, n), dtype=np.float32)
    for k in range(v):
        s, d = seen[:, k], values[:, k]
        with np.errstate(invalid="ignore", over="ignore"):
            if mode == "mean":
                acc = np.where(s, (acc + d).astype(np.float32), acc)
            else:
                better = (d < acc) if mode == "min" else (d > acc)
                acc = np.where(s & (count == 0), d, np.where(s & (count > 0) & better, d, acc))
        count = count + s.astype(np.int32)
        mask = mask | (s.astype(np.uint8) << np.uint8(k))
    valid = count >= min_views
    if mode == "mean":
        with np.errstate(invalid="ignore", divide="ignore"):
            acc = (acc / count.astype(np.float32)).astype(np.float32)
    fused = np.where(valid, acc, np.float32(0.0)).astype(np.float32)
    return fused, mask, valid


def weights(density, seen):
    """density [n, V] float32, seen [n, V] bool -> (w [n, V] float32, W [n] float32) with the fallback applied."""
    density = np.asarray(density, dtype=np.float32)
    w = np.where(np.asarray(seen, dtype=bool), density, np.float32(0.0)).astype(np.float32)
    total = np.zeros(w.shape[0], dtype=np.float32)
    for k in range(w.shape[1]):
        total = (total + w[:, k]).astype(np.float32)
    fallback = ~(total > 0)
    w = np.where(fallback[:, None], np.float32(1.0), w).astype(np.float32)
    total = np.where(fallback, np.float32(w.shape[1]), total).astype(np.float32)
    return w, total


def combine(density, seen, rows):
    """density [n, V], seen [n, V], rows [n, V, D] (float32 per-view outputs) -> the weighted combination [n, D] in float64."""
    w, total = weights(density, seen)
    rows = np.asarray(rows, dtype=np.float64)
    return (w.astype(np.float64)[:, :, None] * rows).sum(axis=1) / total.astype(np.float64)[:, None]


def combine_bound(rows):
    """rows [n, V, D] -> the per-element bound [n, D] of a float32 evaluation against ``combine``."""
    rows = np.asarray(rows, dtype=np.float64)
    v = rows.shape[1]
    return 2.0 * (2 * v + 2) * 2.0 ** -24 * np.abs(rows).max(axis=1)


def views_mask(seen):
    """seen [n, V] bool -> the byte per row with bit v = s_v."""
    seen = np.asarray(seen, dtype=bool)
    out = np.zeros(seen.shape[0], dtype=np.uint8)
    for k in range(seen.shape[1]):
        out |= seen[:, k].astype(np.uint8) << np.uint8(k)
    return out
