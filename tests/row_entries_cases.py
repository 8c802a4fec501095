"""The faulty calls of the four entries that take posed rows or project through cameras -- njf_field_visible, njf_field_frame,
njf_field_tsdf, njf_field_tsdf_sample -- for tests/test_row_entries_cpu.py and tests/golden/make_row_entries_codes.py.

Per entry: the argument names in the order of the C signature, a base call that has NO fault (it is never made), and the single
faults the entries' own CPU tests use -- each pointer missing, each value out of its range, each shape that overflows --, every one
a dict of arguments laid over the base.  ``cases`` yields every single fault and every unordered pair of two faults that set
different arguments (two faults of one argument cannot be laid over each other), but for ``NO_FAULT``.  A grid is written as
``("grid", dims, step, origin)`` and made into the C struct by ``call``; ``P`` stands for a pointer that is never dereferenced,
because every case fails the entry's checks."""
import ctypes as C
import itertools
import math

P = 0x1000
NAN, INF = math.nan, math.inf


def _grid(dims=(5, 4, 3), step=(0.5, 0.5, 0.5), origin=(0.0, 0.0, 0.0)):
    return ("grid", tuple(dims), tuple(step), tuple(origin))


def _faults(pointers, values, shapes, extra=()):
    out = [{key: None} for key in pointers]
    out += [{key: bad} for key, bads in values for bad in bads]
    return out + list(extra) + list(shapes)


_ROW_VALUES = (("num_problems", (0, -1, 65536)), ("num_queries", (0, 2, 4, -3)))
_VIEW_VALUES = (("views", (0, -1, 33)), ("near", (-1.0, NAN, INF)))

ENTRIES = {
    "njf_field_visible": dict(
        names=("points", "count", "labels", "num_queries", "n", "num_problems", "k", "w2c", "views", "height", "width", "footprint",
               "near", "tolerance", "depth", "index", "covered", "seen", "culled", "visible", "pixel", "z", "workspace",
               "workspace_words", "phases"),
        base=dict(num_queries=3, n=500, num_problems=3, views=2, height=48, width=64, footprint=1, near=0.0, tolerance=0.01,
                  workspace_words=2 ** 62, phases=7),
        faults=_faults(
            ("points", "k", "w2c", "depth", "index", "covered", "seen", "culled", "visible", "pixel", "z", "workspace"),
            (("phases", (0, -1, 8, 10, 12, 14, 16, 23)),) + _ROW_VALUES + _VIEW_VALUES +
            (("footprint", (-1, 5, 100)), ("tolerance", (-1e-3, NAN, INF))),
            (dict(n=-1), dict(height=0), dict(width=0), dict(height=-4), dict(height=2 ** 16, width=2 ** 15),
             dict(height=2 ** 14, width=2 ** 14, num_problems=4, num_queries=4), dict(n=2 ** 29, num_problems=2, num_queries=2),
             dict(n=2 ** 30, num_problems=1, num_queries=1), dict(workspace_words=2 * 3 * 2 * 48 * 64))),   # one word short
    ),
    "njf_field_frame": dict(
        names=("points", "count", "labels", "num_queries", "n", "num_problems", "frame", "num_frames", "k", "w2c", "views", "height",
               "width", "reach", "near", "tolerance", "max_distance", "pixel", "z", "state", "index", "distance2", "matched", "found",
               "states", "phases"),
        base=dict(num_queries=3, n=500, num_problems=3, num_frames=3, views=2, height=48, width=64, reach=4, near=0.0, tolerance=0.02,
                  max_distance=0.4, phases=1),
        faults=_faults(
            ("points", "frame", "k", "w2c", "pixel", "z", "state", "index", "distance2", "matched", "found", "states"),
            (("phases", (0, -1, 2, 4, 5, 6, 7, 8, 9, 16)),) + _ROW_VALUES + (("num_frames", (0, 2, 4, -3)),) + _VIEW_VALUES +
            (("reach", (-1, 9, 100)), ("tolerance", (-1e-3, NAN, INF)), ("max_distance", (-0.1, NAN, INF, 1e39))),
            (dict(n=-1), dict(height=0), dict(width=0), dict(height=-4), dict(height=2 ** 16, width=2 ** 15),
             dict(height=2 ** 14, width=2 ** 14, num_frames=3, views=3), dict(height=2 ** 15, width=2 ** 15, views=2, num_frames=1),
             dict(n=2 ** 29, num_problems=2, num_queries=2, num_frames=2),
             dict(n=2 ** 30, num_problems=1, num_queries=1, num_frames=1))),
    ),
    "njf_field_tsdf": dict(
        names=("grid", "depth", "num_problems", "views", "height", "width", "k", "w2c", "near", "far", "truncation", "max_weight",
               "values_in", "weight_in", "values", "weight", "known"),
        base=dict(grid=_grid(), num_problems=3, views=2, height=4, width=64, near=0.0, far=INF, truncation=0.1, max_weight=INF),
        faults=_faults(
            ("grid", "depth", "k", "w2c", "values", "weight", "known", "values_in", "weight_in"),   # (one of the pair without the other)
            (("num_problems", (0, -1, 65536)),) + _VIEW_VALUES +
            (("far", (0.0, -1.0, NAN)), ("truncation", (0.0, -0.1, NAN, INF)), ("max_weight", (0.0, -1.0, NAN))),
            (dict(height=0), dict(height=-1), dict(width=0), dict(grid=_grid((0, 4, 3))), dict(grid=_grid((5, -1, 3))),
             dict(grid=_grid((2048, 1024, 1024))), dict(grid=_grid((1024, 1024, 1024))), dict(height=2 ** 16, width=2 ** 15),
             dict(height=2 ** 14, width=2 ** 14, num_problems=3, views=3), dict(num_problems=2, grid=_grid((1024, 1024, 1024)))),
            extra=(dict(near=0.5, far=0.5),)),
    ),
    "njf_field_tsdf_sample": dict(
        names=("points", "count", "labels", "num_queries", "n", "num_problems", "grid", "values", "weight", "num_fields", "state",
               "distance", "gradient", "states"),
        base=dict(num_queries=3, n=500, num_problems=3, grid=_grid(), num_fields=3),
        faults=_faults(
            ("points", "grid", "values", "weight", "state", "distance", "gradient", "states"),
            _ROW_VALUES + (("num_fields", (0, 2, 4, -3)),),
            (dict(n=-1), dict(grid=_grid((0, 4, 3))), dict(grid=_grid((5, 4, -2))), dict(grid=_grid((2048, 1024, 1024))),
             dict(n=0, grid=_grid((1024, 1024, 1024))), dict(n=2 ** 30, num_problems=2, num_queries=2, num_fields=1),
             dict(n=0, num_problems=2, num_queries=1, num_fields=2, grid=_grid((1024, 1024, 1024)))),
            extra=tuple(dict(grid=g) for g in (
                _grid((1, 4, 3)), _grid((5, 1, 3)), _grid((5, 4, 1)), _grid(step=(0.0, 0.5, 0.5)), _grid(step=(0.5, -0.5, 0.5)),
                _grid(step=(0.5, 0.5, NAN)), _grid(step=(INF, 0.5, 0.5)), _grid(origin=(0.0, INF, 0.0)), _grid(origin=(NAN, 0.0, 0.0))))),
    ),
}


NO_FAULT = dict(values_in=None, weight_in=None)   # njf_field_tsdf without a running state: the one pair that is a valid call


def label(fault: dict) -> str:
    """The name of a fault in the recorded table: its arguments in sorted order."""
    def show(v):
        if isinstance(v, tuple) and v and v[0] == "grid":
            return "grid(" + ";".join(",".join(show(x) for x in part) for part in v[1:]) + ")"
        return repr(v)
    return " ".join(f"{key}={show(fault[key])}" for key in sorted(fault))


def cases(entry: str):
    """(name, arguments laid over the base) of every single fault of ``entry`` and of every pair on different arguments."""
    faults = ENTRIES[entry]["faults"]
    for f in faults:
        yield label(f), f
    for f, g in itertools.combinations(faults, 2):
        if not set(f) & set(g) and {**f, **g} != NO_FAULT:
            yield label(f) + " | " + label(g), {**f, **g}


def call(lib, entry: str, over: dict) -> int:
    """The return code of ``entry`` for the base call with ``over`` laid over it."""
    from neural_jacobian_field_amd import hip
    spec = ENTRIES[entry]
    args = {key: P for key in spec["names"]}
    args.update(spec["base"])
    args.update(over)
    if args.get("grid") is not None:
        _, dims, step, origin = args["grid"]
        args["grid"] = C.byref(hip.make_field_grid(origin, step, dims))
    return getattr(lib, entry)(*[args[key] for key in spec["names"]], None)
