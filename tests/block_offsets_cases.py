"""The workgroup-offsets scan (block_offsets_kernel) restated in plain Python, and the sizes, patterns and
clouds that put it past 256 workgroups through its five callers -- test infrastructure only, shared by
tests/test_block_primitives_cpu.py (which checks that the cases reach the code they are meant for) and the GPU tests of the
selection, the mesh, the band and the cell list (which run them).

The scan, from section 25: one workgroup of THREADS threads over ``blocks`` per-workgroup sums.  Thread t owns the contiguous
run [lo(t), hi(t)) with per = ceil(blocks / THREADS), lo(t) = min(t * per, blocks), hi(t) = min(lo(t) + per, blocks); it adds
its run up, thread 0 scans the THREADS run totals into exclusive run offsets and the grand total, and every thread rewrites its
run with the running sum that starts at its run's offset.  ``offsets`` is that, and with ``mutation`` one of MUTATIONS it is
that with one seam broken; what lies behind the sums (read only by a broken ``hi``) is BEYOND."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "njf_hip.h")
SOURCE = os.path.join(ROOT, "neural-jacobian-field_amd", "csrc", "njf_kernels.hip")


def _define(path, name):
    with open(path) as f:
        return int(re.search(rf"^#define {name} (\d+)\s*$", f.read(), re.M).group(1))


SELECT_BLOCK = _define(HEADER, "NJF_FIELD_SELECT_BLOCK")
MESH_BLOCK = _define(HEADER, "NJF_FIELD_MESH_BLOCK")
BAND_BLOCK = _define(HEADER, "NJF_FIELD_BAND_BLOCK")
SCAN_BLOCK = _define(SOURCE, "NJF_NN_SCAN_BLOCK")
THREADS = _define(SOURCE, "NJF_BLOCK_THREADS")

MUTATIONS = ("no carry inside a run", "no carry from the run scan", "hi not clamped", "the total taken before the last run")
BEYOND = 1           # a word behind the sums: whatever memory holds there, here something that is not zero


# ---- the scan ------------------------------------------------------------------------------------------------------------------------
def workgroups(entries, block):
    return (int(entries) + block - 1) // block


def per_thread(blocks):
    return (blocks + THREADS - 1) // THREADS


def run(blocks, t, clamp_hi=True):
    """(lo, hi) of thread t."""
    per = per_thread(blocks)
    lo = min(t * per, blocks)
    return lo, (min(lo + per, blocks) if clamp_hi else lo + per)


def offsets(sums, mutation=None):
    """(exclusive offsets [blocks], total) of the per-workgroup ``sums`` as the scan's decomposition computes them."""
    assert mutation is None or mutation in MUTATIONS
    sums = [int(v) for v in sums]
    blocks = len(sums)
    read = lambda i: sums[i] if i < blocks else BEYOND                                     # noqa: E731
    runs = [run(blocks, t, clamp_hi=mutation != "hi not clamped") for t in range(THREADS)]
    part = [sum(read(i) for i in range(lo, hi)) for lo, hi in runs]
    start, total = [], 0
    for t in range(THREADS):                                                               # thread 0
        start.append(total)
        if mutation == "the total taken before the last run" and runs[t][0] < blocks and (t + 1 == THREADS or runs[t + 1][0] >= blocks):
            continue                                                                       # the last run that is not empty
        total += part[t]
    out = [None] * blocks
    for t, (lo, hi) in enumerate(runs):
        at = 0 if mutation == "no carry from the run scan" else start[t]
        for i in range(lo, min(hi, blocks)):
            out[i] = at
            if mutation != "no carry inside a run":
                at += read(i)
    return out, total


def seams(sums):
    """Which seams of the decomposition carry a count that is not zero: dict of bool."""
    blocks = len(sums)
    runs = [run(blocks, t) for t in range(THREADS)]
    filled = [r for r in runs if r[0] < r[1]]
    return {"the first sum of a run": any(sums[lo] for lo, hi in filled),
            "a later sum of a run": any(any(sums[lo + 1:hi]) for lo, hi in filled),
            "the last non-empty run": any(sums[filled[-1][0]:filled[-1][1]]),
            "a run that starts at workgroup THREADS or beyond": any(any(sums[lo:hi]) for lo, hi in filled if lo >= THREADS)}


def block_sums(counts, block):
    """The sum of every ``block`` consecutive counts, the last block ragged."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    pad = -counts.size % block
    return np.concatenate([counts, np.zeros(pad, np.int64)]).reshape(-1, block).sum(axis=1)


def regime(blocks):
    """One printed line's worth: what the scan does with ``blocks`` sums."""
    per = per_thread(blocks)
    lengths = [hi - lo for lo, hi in (run(blocks, t) for t in range(THREADS))]
    return dict(workgroups=blocks, per=per, full=sum(n == per for n in lengths), short=sum(0 < n < per for n in lengths),
                empty=sum(n == 0 for n in lengths))


# ---- the selection ---------------------------------------------------------------------------------------------------------------------
# dims -> (entries, workgroups, per, threads with a full run, with a short one, with none): the table of the tests' docstring,
# re-derived from the constants by test_block_primitives_cpu.py
SELECT_GRIDS = {(64, 64, 64): (262144, 256, 1, 256, 0, 0), (65, 64, 64): (266240, 260, 2, 130, 0, 126),
                (67, 66, 65): (287430, 281, 2, 140, 1, 115), (83, 81, 80): (537840, 526, 3, 175, 1, 80)}
SELECT_PATTERNS = ("none", "all", "only the last entry", "the first entry of every workgroup", "the first entry of the odd workgroups",
                   "the entries of workgroups 256 and beyond", "only the last workgroup", "every third entry")


def select_pattern(name, entries):
    """int64 [k] ascending: the kept entries."""
    block, last = SELECT_BLOCK, workgroups(entries, SELECT_BLOCK) - 1
    return {"none": np.zeros(0, np.int64), "all": np.arange(entries), "only the last entry": np.array([entries - 1]),
            "the first entry of every workgroup": np.arange(0, entries, block),
            "the first entry of the odd workgroups": np.arange(block, entries, 2 * block),
            "the entries of workgroups 256 and beyond": np.arange(min(THREADS * block, entries), entries),
            "only the last workgroup": np.arange(last * block, entries), "every third entry": np.arange(0, entries, 3)}[name].astype(np.int64)


LIST_DIMS, LIST_COUNT = (83, 81, 80), 265000        # the list form: every other node, a device count inside workgroup 258 of 263


def select_list():
    """(indices [268,920] int32: every other node; values over the LIST positions; the device count): positions from the count
    on hold values that WOULD pass, so a count that is not honoured shows."""
    indices = np.arange(0, LIST_DIMS[0] * LIST_DIMS[1] * LIST_DIMS[2], 2).astype(np.int32)
    position = np.arange(indices.size)
    values = ((position % 3 == 0) | (position % SELECT_BLOCK == 0)).astype(np.float32)
    values[LIST_COUNT:] = 1.0
    return indices, values, LIST_COUNT


# ---- the mesh and the band -------------------------------------------------------------------------------------------------------------
MESH_CASES = (((67, 66, 65), 1, "sphere"), ((67, 66, 65), 1, "random"), ((53, 52, 53), 2, "random"))       # dims, batch, field
BAND_FACTOR = 8
BAND_CASES = (((65, 65, 73), 1, "random", 1), ((65, 65, 73), 1, "late", 0), ((49, 49, 65), 2, "random", 0),
              ((49, 49, 65), 2, "late", 0))                                                 # dims, batch, hits, dilation
BAND_THRESHOLD = 0.5


def band_values(dims, batch, kind):
    """[B, M] fp32 coarse values (k = BAND_FACTOR) with hits at BAND_THRESHOLD: "random" -- one coarse node in 64, a band that is
    neither empty nor full; "late" -- hits (one node in eight) only on the last coarse x layer of the last element, the last
    tenth of the x range: every offset in front of them is zero."""
    m = tuple((n - 1) // BAND_FACTOR + 1 for n in dims)
    rng = np.random.default_rng(sum(dims) + batch)
    hit = rng.random((batch,) + m) < (1.0 / 8.0 if kind == "late" else 1.0 / 64.0)
    if kind == "late":
        hit[:-1] = False
        hit[-1, :-1] = False
        assert (m[0] - 1) * BAND_FACTOR >= 0.9 * (dims[0] - 1)
    return hit.reshape(batch, -1).astype(np.float32)


# ---- the cell list ---------------------------------------------------------------------------------------------------------------------
CELL_ORIGIN, CELL_SIZE = (-0.37, 0.11, 2.5), 0.043
CELL_CASES = (((67, 66, 65), 1), ((47, 46, 45), 3))                                        # cell dims, clouds
CELL_ROWS, CELL_QUERIES, CELL_REACH = 4097, 512, 6.5 * 0.043                              # ceil(6.5) + 1 = 8 rings of the 64
CRAFTED_FIRST_ROW, CRAFTED_PER_CELL = 10, 2


def crafted_positions(dims, clouds):
    """The list positions (cloud * C + cell) that get points of their own: the ends of the first scan blocks, both sides of
    workgroup THREADS, the seam between two clouds, the last position."""
    c = dims[0] * dims[1] * dims[2]
    at = [0, SCAN_BLOCK - 1, SCAN_BLOCK, 2 * SCAN_BLOCK - 1, 2 * SCAN_BLOCK, THREADS * SCAN_BLOCK - 1, THREADS * SCAN_BLOCK,
          clouds * c - 1]
    return sorted(set(at + ([c - 1, c] if clouds > 1 else [])))


def _uniform(rng, sets, rows, dims, outside):
    extent = np.asarray(dims) * CELL_SIZE
    return (np.asarray(CELL_ORIGIN) + rng.uniform(-outside, 1 + outside, (sets, rows, 3)) * extent).astype(np.float32)


def cell_case(dims, clouds):
    """dict: points [clouds, CELL_ROWS, 3] fp32 -- uniform over the box and 5 % beyond it, three rows that are not finite,
    CRAFTED_PER_CELL points around the centre of every crafted position from row CRAFTED_FIRST_ROW on --, ``crafted``
    [(cloud, row, cell)], queries [clouds, CELL_QUERIES, 3] whose first rows are the crafted centres."""
    rng = np.random.default_rng(sum(dims) + clouds)
    c = dims[0] * dims[1] * dims[2]
    points = _uniform(rng, clouds, CELL_ROWS, dims, 0.05)
    points[:, 3, 1], points[:, CELL_ROWS // 2, 0], points[:, -2] = np.nan, np.inf, -np.inf
    queries = _uniform(rng, clouds, CELL_QUERIES, dims, 0.05)
    crafted, row, query = [], [CRAFTED_FIRST_ROW] * clouds, [0] * clouds
    offset = np.array([0.2, -0.1, 0.15]) * CELL_SIZE
    for position in crafted_positions(dims, clouds):
        cloud, cell = divmod(position, c)
        axis = np.array([cell // (dims[1] * dims[2]), (cell // dims[2]) % dims[1], cell % dims[2]])
        centre = np.asarray(CELL_ORIGIN) + (axis + 0.5) * CELL_SIZE
        for sign in (1.0, -1.0)[:CRAFTED_PER_CELL]:
            points[cloud, row[cloud]] = (centre + sign * offset).astype(np.float32)
            crafted.append((cloud, row[cloud], cell))
            row[cloud] += 1
        queries[cloud, query[cloud]] = (centre + 0.25 * offset).astype(np.float32)
        query[cloud] += 1
    return dict(points=points, queries=queries, crafted=crafted, cells=c, positions=clouds * c)
