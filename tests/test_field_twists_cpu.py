"""Host-side tests of the rigid-twist fit (field_volume.fit_twists / cloud_twists / FieldTwists; njf_field_twists; DESIGN.md
section 15): the numpy restatement (tests/field_twists_restatement.py) against its own node-by-node loop and against
``np.linalg.lstsq`` on the 6-unknown system, planted twists, the conditioning of the fixture, ``screw()``, every argument check
-- raised before any device work: there is no GPU here -- and the C ABI's symbol.

The error of the restatement against twists planted in fp32 is computed by ``planted_error`` of the restatement module: the GPU
test adds its own 1e-9 term to the very same figure."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import field_twists_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8
ARGUMENTS = 28


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


# ---- the fixture and the restatement ------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_issue_describes(fx):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    grid = FieldGrid.from_bounds(R.LOWER, R.UPPER, R.DIMS)
    n, count = fx["labels"].shape[0], fx["count"]
    assert n == count + R.PAD and (np.diff(fx["index"][:count]) > 0).all()
    assert np.array_equal(grid.points(torch.from_numpy(fx["index"][:count])).numpy(), fx["xyz"][:count])      # the grid's own floats
    assert (np.diff(fx["parts"]) > 0).all() and fx["parts"][0] >= 0 and fx["parts"][-1] >= grid.num_nodes     # labels of element 1
    sizes = {name: int((fx["labels"][:count] == p).sum()) for name, p in zip(fx["names"], fx["parts"])}
    assert sizes == {"one node": 1, "collinear": 3, "2x2x2": 8, "one layer": 30, "12x9x7": 756, "16x17x18": 4896}
    assert (fx["labels"][:count] == -1).sum() == 300
    rows = np.flatnonzero(fx["labels"][:count] == fx["parts"][-1])
    assert rows[0] // 4096 != rows[-1] // 4096 and count % 4096 != 0      # a part crosses a chunk boundary, the last chunk is partial
    assert np.isnan(fx["xyz"][count:]).all() and (fx["labels"][count:] == fx["parts"][-1]).all()


def test_the_vectorised_restatement_equals_its_node_by_node_loop(fx):
    rng = np.random.default_rng(3)
    # the small parts and a slice of the big ones (a Python loop per node and channel): relabel a subsample
    keep = np.flatnonzero(fx["labels"][:fx["count"]] >= 0)[::7]
    xyz, labels = fx["xyz"][keep], fx["labels"][keep]
    small = np.flatnonzero(np.isin(fx["labels"][:fx["count"]], fx["parts"][:4]))
    xyz, labels = np.concatenate([fx["xyz"][small], xyz]), np.concatenate([fx["labels"][small], labels])
    jac = rng.normal(size=(xyz.shape[0], 3, 3)).astype(np.float32)
    w = rng.uniform(0.0, 2.0, size=xyz.shape[0]).astype(np.float32)
    w[::5] = 0.0
    w[1::11] = -1.0
    w[2::13] = np.nan
    parts = np.concatenate([fx["parts"], [2 ** 30]]).astype(np.int32)          # the last slot has no rows
    count = xyz.shape[0] - 9
    ref = R.fit(xyz, jac, labels, parts, parts_count=len(parts), count=count, weights=w)
    loop = R.fit_loop(xyz, jac, labels, parts, parts_count=len(parts), count=count, weights=w)
    for p, slot in enumerate(loop):
        for key, value in slot.items():
            assert np.array_equal(np.asarray(ref[key][p]), np.asarray(value)), (p, key)    # the same terms, fsum: bit for bit
    assert ref["status"][-1] == R.EMPTY and ref["nodes"][-1] == 0
    # truncation: parts_count below K fits the first of them, above K reports the true number
    cut = R.fit(xyz, jac, labels, parts, parts_count=2, count=count, weights=w)
    assert (cut["labels"][2:] == -1).all() and not cut["omega"][2:].any() and np.array_equal(cut["omega"][:2], ref["omega"][:2])
    assert R.fit(xyz, jac, labels, parts[:3], parts_count=9, count=count)["count"][0] == 9


def test_the_restatement_equals_least_squares_on_the_six_unknowns(fx):
    """The centred normal equations (v = P / W, omega = M^-1 L) against np.linalg.lstsq on the full 6-unknown system: < 1e-12
    relative on the fixture (measured: 4e-15)."""
    rng = np.random.default_rng(5)
    n, count = fx["labels"].shape[0], fx["count"]
    jac = rng.normal(size=(n, 2, 3)).astype(np.float32)
    w = R.fixture_weights(fx, 6)
    ref = R.fit(fx["xyz"], jac, fx["labels"], fx["parts"], count=count, weights=w)
    worst = 0.0
    for p, name in enumerate(fx["names"]):
        if name in R.DEGENERATE:
            continue
        rows = np.flatnonzero(fx["labels"][:count] == fx["parts"][p])
        ext = R.extent(ref, p)
        for a in range(2):
            om, v = R.lstsq_twist(fx["xyz"][rows], jac[rows, a], w[rows], ref["centroid"][p])
            scale = max(np.linalg.norm(om) * ext, np.linalg.norm(v))
            worst = max(worst, np.linalg.norm(ref["omega"][p, a] - om) * ext / scale, np.linalg.norm(ref["velocity"][p, a] - v) / scale)
    print(f"restatement against lstsq: {worst:.3g}")
    assert worst < 1e-12


def test_planted_twists_come_back(fx):
    """Twists rounded to fp32, Jacobians rounded to fp32: the restatement returns them within 1e-6 relative (measured: 3.6e-8);
    the degenerate parts return the weighted mean as v and omega = 0."""
    worst, (jac, omega, vel, q, w, ref) = R.planted_error(fx)
    print(f"restatement against the planted twists: {worst:.3g}")
    assert worst <= 1e-6
    for p, name in enumerate(fx["names"]):
        assert ref["status"][p] == (R.TRANSLATION if name in R.DEGENERATE else 0), name
        if name in R.DEGENERATE:
            assert not ref["omega"][p].any()
        else:
            assert (ref["residual"][p] <= 1e-12 * ref["energy"][p]).all()       # fp32 rounding of J: 2^-48 of the energy


def test_the_fixture_parts_are_well_conditioned(fx):
    """kappa(M) <= 100 for every non-degenerate fixture part (measured: 3.6), so n * kappa * u ~ 1e-10 in the GPU test."""
    w = R.fixture_weights(fx, 12)
    n = fx["labels"].shape[0]
    ref = R.fit(fx["xyz"], np.zeros((n, 1, 3), np.float32), fx["labels"], fx["parts"], count=fx["count"], weights=w)
    worst = 0.0
    for p, name in enumerate(fx["names"]):
        if name not in R.DEGENERATE:
            worst = max(worst, np.linalg.cond(R.m_matrix(ref["Q"][p])))
    print(f"kappa(M) of the fixture: {worst:.3g}")
    assert worst <= 100


def test_the_pivot_floor_makes_a_line_translation_only_but_not_a_plane():
    line = np.array([[0.1 * i, 0.2 * i, -0.1 * i] for i in range(5)], dtype=np.float32)
    plane = np.array([[0.1 * i, 0.1 * j, 0.0] for i in range(3) for j in range(3)], dtype=np.float32)
    for xyz, status in ((line, R.TRANSLATION), (plane, 0), (line[:1], R.TRANSLATION)):
        jac = np.ones((xyz.shape[0], 1, 3), np.float32)
        ref = R.fit(xyz, jac, np.zeros(xyz.shape[0], np.int32), np.zeros(1, np.int32))
        assert ref["status"][0] == status and np.allclose(ref["velocity"][0, 0], 1.0)


# ---- FieldTwists methods on CPU copies ----------------------------------------------------------------------------------------------
def _twists(omega, velocity, centroid, extent=1.0, energy=None, residual=None):
    from neural_jacobian_field_amd.field_volume import FieldTwists
    k, a = omega.shape[:2]
    f64 = torch.float64
    q = torch.zeros(k, 6, dtype=f64)
    q[:, 0] = extent * extent                      # tr Q / W = extent^2
    z = torch.zeros(k, a, dtype=f64)
    return FieldTwists(labels=torch.arange(k, dtype=torch.int32), count=torch.tensor([k], dtype=torch.int32),
                       nodes=torch.ones(k, dtype=torch.int32), status=torch.zeros(k, dtype=torch.int32), weight=torch.ones(k, dtype=f64),
                       centroid=centroid, omega=omega, velocity=velocity, energy=z + 1 if energy is None else energy,
                       residual=z if residual is None else residual, Q=q, P=velocity.clone(), L=torch.zeros_like(omega),
                       row_residual=torch.zeros(0))


def test_screw_of_a_rotation_a_translation_and_a_known_pitch():
    f64 = torch.float64
    axis = torch.tensor([1.0, 2.0, 2.0], dtype=f64) / 3.0
    on_axis = torch.tensor([0.3, -0.2, 0.5], dtype=f64)
    c = torch.tensor([[1.0, 0.5, -0.25]], dtype=f64)
    rate, pitch = 0.7, 0.125
    rotation = torch.linalg.cross(rate * axis, c[0] - on_axis)                         # v at c of a rotation about the line
    omega = torch.stack([rate * axis, torch.zeros(3, dtype=f64), rate * axis, torch.zeros(3, dtype=f64)])[None]
    velocity = torch.stack([rotation, torch.tensor([0.0, 3.0, 4.0], dtype=f64), rotation + pitch * rate * axis,
                            torch.zeros(3, dtype=f64)])[None]
    direction, point, got_pitch = _twists(omega, velocity, c).screw()
    for a in (0, 2):
        assert torch.allclose(direction[0, a], axis, atol=1e-15)
        foot = on_axis + torch.dot(c[0] - on_axis, axis) * axis                        # the point of the line nearest c
        assert torch.allclose(point[0, a], foot, atol=1e-14)
    assert abs(float(got_pitch[0, 0])) < 1e-15 and abs(float(got_pitch[0, 2]) - pitch) < 1e-15
    assert torch.allclose(direction[0, 1], torch.tensor([0.0, 0.6, 0.8], dtype=f64)) and torch.equal(point[0, 1], c[0])
    assert math.isinf(float(got_pitch[0, 1]))
    assert not direction[0, 3].any() and torch.equal(point[0, 3], c[0])               # a zero twist: no direction, no NaN
    assert not any(torch.isnan(t).any() for t in (direction, point))
    # the prismatic threshold is |omega| * extent <= eps * |v|
    tiny = _twists(omega[:, :1] * 1e-12, velocity[:, 1:2], c)
    assert math.isinf(float(tiny.screw()[2][0, 0])) and math.isfinite(float(tiny.screw(eps=1e-15)[2][0, 0]))


def test_rigidity_and_jacobian_at():
    f64 = torch.float64
    omega = torch.tensor([[[0.0, 0.0, 2.0], [1.0, 0.0, 0.0]]], dtype=f64)
    velocity = torch.tensor([[[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]], dtype=f64)
    tw = _twists(omega, velocity, torch.tensor([[1.0, 1.0, 1.0]], dtype=f64), energy=torch.tensor([[4.0, 0.0]], dtype=f64),
                 residual=torch.tensor([[1.0, 0.0]], dtype=f64))
    assert torch.equal(tw.rigidity(), torch.tensor([[0.75, 1.0]], dtype=f64))
    got = tw.jacobian_at(torch.tensor([[2.0, 1.0, 1.0], [1.0, 3.0, 1.0]]), 0)
    assert got.dtype == f64 and tuple(got.shape) == (2, 2, 3)
    assert torch.equal(got[0], torch.tensor([[1.0, 2.0, 0.0], [0.0, 0.0, 0.0]], dtype=f64))       # v + omega x (1, 0, 0)
    assert torch.equal(got[1], torch.tensor([[-3.0, 0.0, 0.0], [0.0, 0.0, 2.0]], dtype=f64))      # v + omega x (0, 2, 0)


# ---- argument errors ------------------------------------------------------------------------------------------------------------------
def test_fit_twists_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import fit_twists
    n = 6
    xyz, jac = torch.zeros(n, 3), torch.zeros(n, 4, 3)
    labels, parts = torch.zeros(n, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    one = torch.ones(1, dtype=torch.int32)
    for bad in (xyz.double(), torch.zeros(n, 2), torch.zeros(3 * n), None):
        with pytest.raises(ValueError, match="xyz must be"):
            fit_twists(bad, jac, labels, parts)
    for bad in (jac.double(), torch.zeros(n + 1, 4, 3), torch.zeros(n, 4, 2), torch.zeros(n, 0, 3), torch.zeros(n, 12)):
        with pytest.raises(ValueError, match="jacobian must be"):
            fit_twists(xyz, bad, labels, parts)
    with pytest.raises(ValueError, match="at most 10 command channels"):
        fit_twists(xyz, torch.zeros(n, 11, 3), labels, parts)
    for bad in (labels.long(), labels[:-1], labels.reshape(1, n)):
        with pytest.raises(ValueError, match="labels must be int32"):
            fit_twists(xyz, jac, bad, parts)
    for bad in (parts.long(), parts.reshape(1, 2)):
        with pytest.raises(ValueError, match="parts must be int32"):
            fit_twists(xyz, jac, labels, bad)
    for bad in (torch.zeros(0, dtype=torch.int32), torch.zeros(257, dtype=torch.int32)):
        with pytest.raises(ValueError, match="1 to 256 labels"):
            fit_twists(xyz, jac, labels, bad)
    for bad in (torch.zeros(n, dtype=torch.float64), torch.zeros(n - 1), "density"):
        with pytest.raises(ValueError, match="weights must be fp32"):
            fit_twists(xyz, jac, labels, parts, weights=bad)
    for key in ("count", "parts_count"):
        for bad in (3, torch.ones(2, dtype=torch.int32), torch.ones(1)):
            with pytest.raises(ValueError, match=f"{key} must be one int32"):
                fit_twists(xyz, jac, labels, parts, **{key: bad})
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="must live on the device"):
            fit_twists(xyz.cuda(), jac, labels, parts)
    with pytest.raises(ValueError, match="no CPU path"):
        fit_twists(xyz, jac, labels, parts, count=one, parts_count=one, weights=torch.ones(n))


def test_cloud_twists_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud, cloud_twists
    n = 5
    grid = FieldGrid.from_bounds(R.LOWER, R.UPPER, (3, 3, 3))

    def cloud(a=4, jacobian=True):
        return FieldPointCloud(grid=grid, index=torch.arange(n, dtype=torch.int32), xyz=torch.zeros(n, 3), density=torch.ones(n),
                               color=None, jacobian=torch.zeros(n, a, 3) if jacobian else None,
                               count=torch.tensor([n], dtype=torch.int32))

    labels = torch.zeros(n, dtype=torch.int32)
    with pytest.raises(ValueError, match="needs the Jacobians"):
        cloud_twists(cloud(jacobian=False))
    for bad in (0, 257, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="max_parts must be"):
            cloud_twists(cloud(), max_parts=bad)
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError, match="min_nodes must be"):
            cloud_twists(cloud(), min_nodes=bad)
    with pytest.raises(ValueError, match="connectivity must be 6 or 14"):
        cloud_twists(cloud(), connectivity=26)
    with pytest.raises(ValueError, match="at most 10 command channels"):
        cloud_twists(cloud(a=11))
    with pytest.raises(ValueError, match="come together"):
        cloud_twists(cloud(), labels=labels)
    for bad in (labels.long(), labels[:-1]):
        with pytest.raises(ValueError, match="labels must be int32"):
            cloud_twists(cloud(), labels=bad, sizes=labels)
        with pytest.raises(ValueError, match="sizes must be int32"):
            cloud_twists(cloud(), labels=labels, sizes=bad)
    for bad in ("uniform", torch.ones(n - 1), torch.ones(n, dtype=torch.float64)):
        with pytest.raises(ValueError, match="weights must be"):
            cloud_twists(cloud(), labels=labels, sizes=labels, weights=bad)
    with pytest.raises(ValueError, match="no CPU path"):
        cloud_twists(cloud(), labels=labels, sizes=labels, weights=None)
    with pytest.raises(ValueError, match="no CPU path"):
        cloud_twists(cloud())


def test_the_signatures():
    from neural_jacobian_field_amd import field_volume
    params = inspect.signature(field_volume.fit_twists).parameters
    assert list(params) == ["xyz", "jacobian", "labels", "parts", "parts_count", "count", "weights"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None for k in ("parts_count", "count", "weights"))
    params = inspect.signature(field_volume.cloud_twists).parameters
    defaults = dict(labels=None, sizes=None, connectivity=6, keys=None, min_nodes=1, max_parts=32, weights="density", batch=None)
    assert {k: params[k].default for k in defaults} == defaults
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in defaults)
    assert list(field_volume.FieldTwists.__dataclass_fields__) == [
        "labels", "count", "nodes", "status", "weight", "centroid", "omega", "velocity", "energy", "residual", "Q", "P", "L", "row_residual"]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "njf_field_twists" in declared and "njf_field_twists" in hip.EXPORTED_SYMBOLS and hasattr(lib, "njf_field_twists")
    params = re.search(r"njf_field_twists\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(lib.njf_field_twists.argtypes) == ARGUMENTS
    assert lib.njf_abi_version() == 20          # the change is additive
    defines = {k: int(v) for k, v in re.findall(r"#define (NJF_FIELD_TWISTS_[A-Z_]+) (\d+)", header)}
    assert defines["NJF_FIELD_TWISTS_CHUNK"] == hip.FIELD_TWISTS_CHUNK == 4096
    assert defines["NJF_FIELD_TWISTS_MAX_PARTS"] == hip.FIELD_TWISTS_MAX_PARTS == 256
    assert (defines["NJF_FIELD_TWISTS_EMPTY"], defines["NJF_FIELD_TWISTS_TRANSLATION"]) == (hip.FIELD_TWISTS_EMPTY,
                                                                                         hip.FIELD_TWISTS_TRANSLATION) == (R.EMPTY, R.TRANSLATION)
    assert defines["NJF_FIELD_TWISTS_ALL"] == hip.FIELD_TWISTS_ALL == sum(hip.FIELD_TWISTS_PHASES)
    assert len(hip.FIELD_TWISTS_PHASES) == len(hip.FIELD_TWISTS_PHASE_NAMES)
    assert hip.field_twists_workspace(4097, 3, 10) == 76 * 3 * 2 and hip.field_twists_workspace(0, 3, 10) == 0


def test_the_c_entry_refuses_bad_arguments_without_a_gpu(lib):
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    names = ("xyz", "jacobian", "labels", "weights", "count", "n", "action_dim", "parts", "parts_count", "num_parts", "out_labels",
             "out_count", "nodes", "status", "weight", "centroid", "omega", "velocity", "energy", "residual", "q", "p", "l",
             "row_residual", "workspace", "workspace_doubles", "phases")
    assert len(names) + 1 == ARGUMENTS

    def call(**kw):
        args = {k: P for k in names}
        args.update(n=5000, action_dim=8, num_parts=4, workspace_doubles=4 * 2 * 62, phases=127)
        args.update(kw)
        return lib.njf_field_twists(*[args[k] for k in names], None)

    for bad in (0, -1, 11):
        assert call(action_dim=bad) == E_VALUE
    for bad in (0, -3, 257):
        assert call(num_parts=bad) == E_VALUE
    for bad in (0, -1, 128):
        assert call(phases=bad) == E_VALUE
    assert call(n=-1) == E_SHAPE
    assert call(workspace_doubles=4 * 2 * 62 - 1) == E_SHAPE                    # the workspace is too small
    assert call(n=2 ** 31 - 1, num_parts=256, action_dim=10, workspace_doubles=2 ** 62) == E_SHAPE     # K * chunks * stride overflows
    for key in names:
        if key in ("weights", "count", "parts_count", "n", "action_dim", "num_parts", "workspace_doubles", "phases"):
            continue                                                            # (optional pointers, integers)
        assert call(**{key: None}) == E_NULL, key
    # the rows may be absent when there are none, the outputs may not
    assert call(n=0, workspace_doubles=0, out_labels=None) == E_NULL
