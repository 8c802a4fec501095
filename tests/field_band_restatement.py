"""numpy restatement of the coarse-to-fine band, written from that text: what the GPU tests compare
``band_from_values`` / ``band_leaks`` / the ``coarse`` keyword of the extractions with, bit for bit.

The fine grid has dims (nx, ny, nz) with (n_c - 1) % k == 0; m_c = (n_c - 1) / k blocks and m_c + 1 coarse nodes per axis.
Everything is per batch element: arrays are [B, ...] with nodes and blocks in the linear order (x*ny + y)*nz + z."""
import numpy as np

FACTORS = (2, 4, 8, 16)
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))   # the mesh table of section 11


def blocks_per_axis(dims, k):
    assert k in FACTORS and all((n - 1) % k == 0 and n >= k + 1 for n in dims), (dims, k)
    return tuple((n - 1) // k for n in dims)


def hits(values, threshold, valid=None):
    """[B, M] bool: valid and value >= threshold (NaN compares false; equal is a hit)."""
    with np.errstate(invalid="ignore"):
        hit = np.asarray(values, dtype=np.float32) >= np.float32(threshold)
    return hit if valid is None else hit & (np.asarray(valid) != 0)


def blocks(hit, dims, k, d):
    """[B, Nb] bool: block j is active iff a coarse node q with max(0, j_c - d) <= q_c <= min(m_c, j_c + 1 + d) on every axis
    is a hit."""
    m = blocks_per_axis(dims, k)
    h = np.asarray(hit, dtype=bool).reshape((-1,) + tuple(mc + 1 for mc in m))
    # d layers of "no hit" around the coarse lattice do the clipping: q_c = j_c - d + o_c, o_c = 0 .. 2d + 1
    padded = np.pad(h, ((0, 0),) + ((d, d),) * 3, constant_values=False)
    active = np.zeros((h.shape[0],) + m, dtype=bool)
    for ox in range(2 * d + 2):
        for oy in range(2 * d + 2):
            for oz in range(2 * d + 2):
                active |= padded[:, ox:ox + m[0], oy:oy + m[1], oz:oz + m[2]]
    return active.reshape(h.shape[0], -1)


def band(active, dims, k):
    """[B, N] bool: node i is in the band iff an active block j has j_c*k <= i_c <= (j_c + 1)*k on every axis."""
    m = blocks_per_axis(dims, k)
    a = np.asarray(active, dtype=bool).reshape((-1,) + m).astype(np.int64)
    member = []
    for n, mc in zip(dims, m):
        i, j = np.arange(n)[:, None], np.arange(mc)[None, :]
        member.append(((j * k <= i) & (i <= (j + 1) * k)).astype(np.int64))          # [n_c, m_c]
    inside = np.einsum("bxyz,ix,jy,kz->bijk", a, *member) > 0
    return inside.reshape(a.shape[0], -1)


def band_list(in_band):
    """Ascending global indices b*N + n of the band nodes."""
    return np.flatnonzero(np.asarray(in_band, dtype=bool).reshape(-1)).astype(np.int64)


def leaks(inside, in_band, dims):
    """The number of inside nodes with a neighbour g +- direction, inside the grid and the same element, that is not in the band."""
    b = np.asarray(inside).shape[0]
    ins = np.asarray(inside, dtype=bool).reshape((b,) + tuple(dims))
    out = ~np.asarray(in_band, dtype=bool).reshape((b,) + tuple(dims))
    leak = np.zeros_like(ins)
    nx, ny, nz = dims
    for dx, dy, dz in DIRECTIONS:
        lo = (slice(None), slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))       # nodes that have g + dir
        hi = (slice(None), slice(dx, nx), slice(dy, ny), slice(dz, nz))                   # nodes that have g - dir
        leak[lo] |= out[hi]
        leak[hi] |= out[lo]
    return int((leak & ins).sum())


def full(values, valid, threshold, dims, k, d):
    """(active [B, Nb], band [B, N], list, count) from coarse values."""
    active = blocks(hits(values, threshold, valid), dims, k, d)
    in_band = band(active, dims, k)
    index = band_list(in_band)
    return active, in_band, index, index.size
