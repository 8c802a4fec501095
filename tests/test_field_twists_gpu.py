"""GPU tests of the rigid-twist fit (field_volume.fit_twists / cloud_twists; njf_field_twists) against
the float64 numpy restatement of its semantics (tests/field_twists_restatement.py).

The bounds, all stated before anything ran (u = 2^-53; m = the rows of positive weight of a part = the terms of each sum):

1. every raw sum s = sum t_i (W, Q, P, L, E):  |s_gpu - s_ref| <= 2 m u sum|t_i|.  The terms are bit-identical by construction
   (the same IEEE operations in the same order on the same fp32 inputs), the reference sum is correctly rounded (fsum), so only
   the device's summation order differs, and this is its first-order bound.  Pass B is formed around the centroid the GPU
   returned, because those sums are defined relative to it.  The centroid c = S / W gets the same bound propagated through
   the quotient: 2 (m + 1) u (sum|w x| / W + |c|) per component (one more rounding for the division).
2. omega against ``np.linalg.solve`` on the GPU's own M, L: <= 64 kappa(M) u max|omega| per channel; omega and v against the
   restatement end to end: <= 1e-9 max(|omega| extent, |v|) in velocity units (an omega error times the extent), extent =
   sqrt(tr Q / W): n <= 1e4 terms, kappa <= 1e2, u = 1.1e-16 give n kappa u ~ 1e-10, with a tenfold margin; an fp32
   accumulation misses it by three orders of magnitude.
3. residual within 1e-9 energy of the restatement's direct residual; row_residual (fp32) within 2^-22 of its value.

Run with -m gpu."""
import math

import numpy as np
import pytest
import torch

import field_components_restatement as RC
import field_twists_restatement as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
IMG = 64
FIELDS = ("labels", "count", "nodes", "status", "weight", "centroid", "omega", "velocity", "energy", "residual", "Q", "P", "L",
          "row_residual")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def planted(fx):
    """The planted field and the restatement's own error against the plant: computed once, shared, never changed."""
    return R.planted_error(fx)


def _grid(dims=R.DIMS):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds(R.LOWER, R.UPPER, dims)


def _np(tw):
    return {f: getattr(tw, f).cpu().numpy() for f in FIELDS}


def _dev(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _one(dev, v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=dev)


def _fit(dev, xyz, jac, labels, parts, parts_count=None, count=None, weights=None):
    from neural_jacobian_field_amd.field_volume import fit_twists
    tw = fit_twists(_dev(dev, xyz), _dev(dev, jac), _dev(dev, labels), _dev(dev, parts), parts_count=_one(dev, parts_count),
                    count=_one(dev, count), weights=_dev(dev, weights))
    k, a, n = len(parts), jac.shape[1], xyz.shape[0]
    shapes = dict(labels=(k,), count=(1,), nodes=(k,), status=(k,), weight=(k,), centroid=(k, 3), omega=(k, a, 3), velocity=(k, a, 3),
                  energy=(k, a), residual=(k, a), Q=(k, 6), P=(k, a, 3), L=(k, a, 3), row_residual=(n,))
    for f, shape in shapes.items():
        t = getattr(tw, f)
        want = torch.int32 if f in ("labels", "count", "nodes", "status") else torch.float32 if f == "row_residual" else torch.float64
        assert tuple(t.shape) == shape and t.dtype == want and t.device.type == "cuda", f
    return tw


def _check(got, xyz, jac, labels, parts, parts_count=None, count=None, weights=None, kappa_limit=None, rows_exact=True):
    """Bounds 1-3 of the module docstring on one result (numpy dict).  ``kappa_limit``: apply the solve bounds only to the
    parts with kappa(M) <= the limit.  Returns the restatement and the slots the solve bounds were applied to."""
    ref = R.fit(xyz, jac, labels, parts, parts_count, count, weights)
    around = R.fit(xyz, jac, labels, parts, parts_count, count, weights, centroid=got["centroid"])
    for f in ("labels", "count", "nodes", "status"):
        assert np.array_equal(got[f], ref[f]), (f, got[f], ref[f])
    k, a_dim = len(parts), jac.shape[1]
    solved = []
    worst = dict(sums=0.0, solve=0.0, end=0.0)
    for p in range(k):
        if ref["labels"][p] < 0 or ref["status"][p] & R.EMPTY:
            for f in ("weight", "centroid", "omega", "velocity", "energy", "residual", "Q", "P", "L"):
                assert not got[f][p].any(), (p, f)                          # an unused or empty slot is zero
            continue
        m = int(ref["terms"][p])
        order = 2.0 * m * U
        assert abs(got["weight"][p] - ref["weight"][p]) <= order * ref["abs"]["W"][p], (p, "W")
        for d in range(3):
            c = ref["centroid"][p, d]
            bound = 2.0 * (m + 1) * U * (ref["abs"]["S"][p, d] / ref["weight"][p] + abs(c))
            assert abs(got["centroid"][p, d] - c) <= bound, (p, "centroid", d, got["centroid"][p, d] - c, bound)
        for f, key in (("Q", "Q"), ("P", "P"), ("L", "L"), ("energy", "E")):
            err, bound = np.abs(got[f][p] - around[f][p]), order * around["abs"][key][p]
            assert (err <= bound).all(), (p, f, err.max(), bound.min())
            worst["sums"] = max(worst["sums"], float((err / np.maximum(bound, 1e-300)).max()))
        ext = R.extent(ref, p)
        matrix = R.m_matrix(got["Q"][p])
        if ref["status"][p] & R.TRANSLATION:
            assert not got["omega"][p].any(), p
            assert np.abs(got["velocity"][p] - ref["velocity"][p]).max() <= 1e-9 * np.abs(ref["velocity"][p]).max(), p
        else:
            kappa = np.linalg.cond(matrix)
            if kappa_limit is None or kappa <= kappa_limit:
                solved.append(p)
                direct = np.linalg.solve(matrix, got["L"][p].T).T
                for a in range(a_dim):
                    err, bound = np.abs(got["omega"][p, a] - direct[a]).max(), 64.0 * kappa * U * np.abs(direct[a]).max()
                    assert err <= bound, (p, a, "omega against linalg.solve", err, bound)
                    worst["solve"] = max(worst["solve"], err / bound)
                    scale = max(np.linalg.norm(ref["omega"][p, a]) * ext, np.linalg.norm(ref["velocity"][p, a]))
                    e_om = np.linalg.norm(got["omega"][p, a] - ref["omega"][p, a]) * ext
                    e_v = np.linalg.norm(got["velocity"][p, a] - ref["velocity"][p, a])
                    assert max(e_om, e_v) <= 1e-9 * scale, (p, a, "end to end", e_om, e_v, scale)
                    worst["end"] = max(worst["end"], max(e_om, e_v) / scale)
                assert (np.abs(got["residual"][p] - ref["residual"][p]) <= 1e-9 * ref["energy"][p]).all(), (p, "residual")
    # rows of no fitted part, and rows past the count, have row_residual 0; the others the restatement's value in fp32
    rows = xyz.shape[0] if count is None else count
    fitted = np.zeros(xyz.shape[0], dtype=bool)
    fitted[:rows] = np.isin(labels[:rows], ref["labels"][ref["labels"] >= 0])
    assert not got["row_residual"][~fitted].any()
    if rows_exact:
        want = ref["row_residual"].astype(np.float64)
        assert np.array_equal(np.isnan(got["row_residual"]), np.isnan(want))
        finite = ~np.isnan(want)
        assert (np.abs(got["row_residual"][finite] - want[finite]) <= 2.0 ** -22 * np.abs(want[finite])).all()
    print("share of the bounds used:", {key: f"{v:.3g}" for key, v in worst.items()}, "parts solved:", solved)
    return ref, solved


# ---- 3. a planted rigid field -------------------------------------------------------------------------------------------------------
def test_a_planted_rigid_field_comes_back(dev, fx, planted):
    worst_ref, (jac, omega, vel, q, w, _) = planted
    assert worst_ref <= 1e-6
    tw = _fit(dev, fx["xyz"], jac, fx["labels"], fx["parts"], count=fx["count"], weights=w)
    got = _np(tw)
    # (the row residual of a rigid field is rounding noise: its relative error says nothing, bound 3 applies to test 4)
    ref, solved = _check(got, fx["xyz"], jac, fx["labels"], fx["parts"], count=fx["count"], weights=w, rows_exact=False)
    assert [fx["names"][p] for p in solved] == [n for n in fx["names"] if n not in R.DEGENERATE]
    worst = 0.0
    for p, name in enumerate(fx["names"]):
        if name in R.DEGENERATE:
            assert got["status"][p] == R.TRANSLATION and not got["omega"][p].any()
            continue
        assert got["status"][p] == 0
        ext = R.extent(ref, p)
        v_at_c = vel[p] + np.cross(omega[p], ref["centroid"][p] - q[p])
        for a in range(3):
            scale = max(np.linalg.norm(omega[p, a]) * ext, np.linalg.norm(v_at_c[a]))
            worst = max(worst, np.linalg.norm(got["omega"][p, a] - omega[p, a]) * ext / scale,
                        np.linalg.norm(got["velocity"][p, a] - v_at_c[a]) / scale)
        assert (tw.rigidity()[p] > 1 - 1e-9).all(), name
    print(f"against the plant: GPU {worst:.3g}, restatement {worst_ref:.3g}")
    assert worst <= worst_ref + 1e-9
    # the degenerate parts: v is the weighted mean of J
    count = fx["count"]
    for p, name in enumerate(fx["names"]):
        if name in R.DEGENERATE:
            rows = np.flatnonzero(fx["labels"][:count] == fx["parts"][p])
            mean = (w[rows].astype(np.float64)[:, None, None] * jac[rows].astype(np.float64)).sum(0) / w[rows].astype(np.float64).sum()
            assert np.abs(got["velocity"][p] - mean).max() <= 1e-12 * np.abs(mean).max()


# ---- 4. a non-rigid field, zero weights, NaN under zero weights, an empty part ------------------------------------------------------
def _non_rigid(fx, a_dim, seed):
    rng = np.random.default_rng(seed)
    n, count = fx["labels"].shape[0], fx["count"]
    jac = rng.normal(size=(n, a_dim, 3)).astype(np.float32)
    w = rng.lognormal(0.0, 1.0, size=n).astype(np.float32)                  # density-like
    zero = rng.random(n) < 0.1
    w[zero] = 0.0
    w[np.flatnonzero(zero)[::3]] = -1.0
    w[np.flatnonzero(zero)[1::3]] = np.nan
    xyz = fx["xyz"].copy()
    poisoned = np.flatnonzero(zero)
    xyz[poisoned[::2], 1] = np.nan                                           # harmless: these rows enter no sum
    jac[poisoned[1::2], a_dim // 2, 2] = np.nan
    empty = fx["names"].index("2x2x2")
    w[fx["labels"] == fx["parts"][empty]] = 0.0
    assert count < n
    return xyz, jac, w, empty


def test_a_non_rigid_field_with_zero_weights_and_an_empty_part(dev, fx):
    xyz, jac, w, empty = _non_rigid(fx, 10, 21)
    tw = _fit(dev, xyz, jac, fx["labels"], fx["parts"], count=fx["count"], weights=w)
    got = _np(tw)
    ref, solved = _check(got, xyz, jac, fx["labels"], fx["parts"], count=fx["count"], weights=w)
    assert got["status"][empty] == R.EMPTY and got["nodes"][empty] == 8 and len(solved) == 3
    assert (got["nodes"] > ref["terms"]).any()                               # rows of weight 0 count as nodes
    assert np.isnan(got["row_residual"]).any()                               # ... and a NaN under a zero weight stays in its row only
    assert not any(np.isnan(got[f]).any() for f in FIELDS if f != "row_residual")
    rigidity = tw.rigidity().cpu().numpy()
    # noise is not rigid: six parameters against 3 m_eff numbers, m_eff = (sum w)^2 / sum w^2 ~ m / e for these weights, explain
    # about 2 e / m of it -- below 0.01 for the two boxes of 756 and 4,896 nodes (the 30-node layer is too small to say);
    # a part without energy has rigidity 1 by definition
    big = [p for p in solved if got["nodes"][p] >= 500]
    assert len(big) == 2 and (rigidity[big] < 0.1).all() and (rigidity[empty] == 1.0).all()
    # sum w row_residual = the residual summed over the channels (row_residual is fp32: 1e-6 of the energy)
    weights = R.effective_weights(w, w.shape[0])
    for p in solved:
        rows = np.flatnonzero((fx["labels"][:fx["count"]] == fx["parts"][p]) & (weights[:fx["count"]] > 0))
        total = math.fsum((weights[rows] * got["row_residual"][rows].astype(np.float64)).tolist())
        assert abs(total - got["residual"][p].sum()) <= 1e-6 * got["energy"][p].sum(), p


# ---- 5. one channel -----------------------------------------------------------------------------------------------------------------
def test_one_channel(dev, fx):
    xyz, jac, w, _ = _non_rigid(fx, 1, 22)
    got = _np(_fit(dev, xyz, jac, fx["labels"], fx["parts"], count=fx["count"], weights=w))
    _check(got, xyz, jac, fx["labels"], fx["parts"], count=fx["count"], weights=w)
    # and without weights: every row counts once
    jac = np.nan_to_num(jac)
    got = _np(_fit(dev, fx["xyz"], jac, fx["labels"], fx["parts"], count=fx["count"]))
    ref, _ = _check(got, fx["xyz"], jac, fx["labels"], fx["parts"], count=fx["count"])
    assert np.array_equal(got["weight"], got["nodes"].astype(np.float64)) and np.array_equal(ref["terms"], got["nodes"])


# ---- 6. capacity and truncation ------------------------------------------------------------------------------------------------------
def _cloud(dev, fx, jac, density):
    from neural_jacobian_field_amd.field_volume import FieldPointCloud
    return FieldPointCloud(grid=_grid(), index=_dev(dev, fx["index"]), xyz=_dev(dev, fx["xyz"]), density=_dev(dev, density),
                           color=None, jacobian=_dev(dev, jac), count=_one(dev, fx["count"]))


def _sizes(fx):
    labels, count = fx["labels"], fx["count"]
    sizes = np.zeros(labels.shape[0], dtype=np.int32)
    for p in fx["parts"]:
        sizes[:count][labels[:count] == p] = (labels[:count] == p).sum()
    return sizes


def test_capacity_and_truncation(dev, fx):
    from neural_jacobian_field_amd.field_volume import cloud_twists
    rng = np.random.default_rng(31)
    n, count = fx["labels"].shape[0], fx["count"]
    jac = rng.normal(size=(n, 4, 3)).astype(np.float32)
    density = rng.lognormal(0.0, 0.5, size=n).astype(np.float32)
    cloud = _cloud(dev, fx, jac, density)
    labels, sizes = _dev(dev, fx["labels"]), _dev(dev, _sizes(fx))
    qualifying = np.array([p for p in fx["parts"] if (fx["labels"][:count] == p).sum() >= 2], dtype=np.int32)
    assert qualifying.size == 5
    # two slots for five parts: the first two ascending labels, the true count
    got = _np(cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=2, max_parts=2))
    assert got["count"][0] == 5 and np.array_equal(got["labels"], qualifying[:2])
    _check(got, fx["xyz"], jac, fx["labels"], qualifying[:2], parts_count=5, count=count, weights=density)
    # eight slots for five parts: slots 5..7 are unused
    got = _np(cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=2, max_parts=8, weights=None))
    assert got["count"][0] == 5 and np.array_equal(got["labels"], np.concatenate([qualifying, [-1] * 3]))
    parts8 = np.concatenate([qualifying, [-1] * 3]).astype(np.int32)
    _check(got, fx["xyz"], jac, fx["labels"], parts8, parts_count=5, count=count)
    for f in FIELDS[4:-1]:
        assert not got[f][5:].any(), f
    assert not got["nodes"][5:].any() and not got["status"][5:].any()
    # a tensor of weights, all six parts; then a smaller count moves the tail of the last part out of the fit
    got = _np(cloud_twists(cloud, labels=labels, sizes=sizes, weights=_dev(dev, density * 2)))
    assert got["count"][0] == 6 and tuple(got["labels"].shape) == (32,)
    short = count - 1000
    got = _np(_fit(dev, fx["xyz"], jac, fx["labels"], fx["parts"], count=short, weights=density))
    ref, _ = _check(got, fx["xyz"], jac, fx["labels"], fx["parts"], count=short, weights=density)
    assert got["nodes"][-1] == 4896 - 1000 + int((fx["labels"][short:count] != fx["parts"][-1]).sum())
    # a count past the rows reads the rows only (the padding included: give it clean coordinates)
    xyz = np.nan_to_num(fx["xyz"])
    got = _np(_fit(dev, xyz, jac, fx["labels"], fx["parts"], count=n + 5, parts_count=99))
    _check(got, xyz, jac, fx["labels"], fx["parts"], count=n, parts_count=99)
    assert got["count"][0] == 99 and got["nodes"][-1] == 4896 + R.PAD


# ---- 7. determinism and capture ------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_a_capture_replays_them(dev, fx):
    from neural_jacobian_field_amd.field_volume import cloud_twists
    xyz, jac, w, _ = _non_rigid(fx, 7, 41)
    a, b = (_fit(dev, xyz, jac, fx["labels"], fx["parts"], count=fx["count"], weights=w) for _ in range(2))
    for f in FIELDS:
        assert torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f
    # cloud_twists, components and part list included, on one stream: an eager call, then a capture of the same call
    density = np.abs(np.nan_to_num(w)) + 0.5
    cloud = _cloud(dev, fx, np.nan_to_num(jac), density.astype(np.float32))
    kw = dict(min_nodes=2, max_parts=8, batch=2)
    eager = cloud_twists(cloud, **kw)
    assert int(eager.count.item()) >= 4
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = cloud_twists(cloud, **kw)
    for f in FIELDS:
        getattr(captured, f).zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f in FIELDS:
        assert torch.equal(getattr(captured, f).view(torch.uint8), getattr(eager, f).view(torch.uint8)), f


# ---- 8. end to end: a model's field, segmented by the joint that moves a node most ---------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model
    cfg = model_cfg_from_dict({"action_dim": 8, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                               "action_decoder": {"name": "jacobian_mlp"}})
    m = Model(cfg)
    m.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", 8), seed=0), strict=True)
    return m.to(dev).eval().requires_grad_(False)


def _encoding(batch, dev, seed=1):
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.decoder import PixelEncoding
    c2w = synthetic.general_pose(7, batch, scale=0.04)
    c2w[0] = torch.eye(4)
    k = synthetic.synthetic_cameras(batch)["ctxt_k_norm"]
    return PixelEncoding(features=synthetic.synthetic_features(batch, IMG, IMG, seed=seed).to(dev), extrinsics=c2w.to(dev),
                         intrinsics=k.to(dev), action=synthetic.synthetic_action(batch, 8).to(dev))


def test_cloud_twists_end_to_end(model, dev):
    from neural_jacobian_field_amd.field_volume import cloud_components, cloud_twists, dominant_joint, extract_field, fit_twists
    grid = _grid((17, 13, 11))
    enc = _encoding(2, dev)
    xyz_all = grid.points(device=dev)
    head, _ = model.compute_density(xyz_all[None].expand(2, -1, 3).contiguous(), enc)
    dense = head.density.reshape(-1).double().cpu()
    chosen = None
    for quantile in (0.6, 0.75, 0.45, 0.85, 0.3, 0.93):
        cloud = extract_field(model, enc, grid, float(torch.quantile(dense, quantile)))
        n = cloud.index.shape[0]
        if n < 20:
            continue
        keys = dominant_joint(cloud.jacobian)
        # the components restated on the CPU, and the conditioning of the parts of at least 8 nodes
        index = cloud.index.cpu().numpy().astype(np.int64)
        inside = np.zeros(2 * grid.num_nodes, dtype=bool)
        inside[index] = True
        dense_keys = np.zeros(2 * grid.num_nodes, dtype=np.int32)
        dense_keys[index] = keys.cpu().numpy()
        labels, sizes, _ = RC.label(inside.reshape(2, -1), grid.dims, 6, dense_keys.reshape(2, -1))
        labels, sizes = labels.reshape(-1)[index].astype(np.int32), sizes.reshape(-1)[index].astype(np.int32)
        parts = np.unique(labels[sizes >= 8]).astype(np.int32)
        if not 2 <= parts.size <= 32:
            continue
        xyz, jac, density = cloud.xyz.cpu().numpy(), cloud.jacobian.cpu().numpy(), cloud.density.cpu().numpy()
        ref = R.fit(xyz, jac, labels, parts, weights=density)
        good = [p for p in range(parts.size) if ref["status"][p] == 0 and np.linalg.cond(R.m_matrix(ref["Q"][p])) <= 100]
        if len(good) >= 2:
            chosen = (quantile, cloud, keys, labels, sizes, parts, xyz, jac, density, good)
            break
    assert chosen is not None, "no quantile of the list leaves two well-conditioned parts of 8 nodes"
    quantile, cloud, keys, labels, sizes, parts, xyz, jac, density, good = chosen
    tw = cloud_twists(cloud, keys=keys, min_nodes=8)
    got_labels, got_sizes, _ = cloud_components(cloud, keys=keys)
    assert np.array_equal(got_labels.cpu().numpy(), labels) and np.array_equal(got_sizes.cpu().numpy(), sizes)
    padded = np.concatenate([parts, np.full(32 - parts.size, -1, dtype=np.int32)])
    by_hand = fit_twists(cloud.xyz, cloud.jacobian, got_labels, _dev(dev, padded), parts_count=_one(dev, int(parts.size)),
                         count=cloud.count, weights=cloud.density)
    for f in FIELDS:
        assert torch.equal(getattr(tw, f).view(torch.uint8), getattr(by_hand, f).view(torch.uint8)), f
    _, solved = _check(_np(tw), xyz, jac, labels, padded, parts_count=int(parts.size), count=xyz.shape[0], weights=density,
                       kappa_limit=100)
    print(f"quantile {quantile}: {xyz.shape[0]} rows, {parts.size} parts of at least 8 nodes, {len(solved)} with kappa(M) <= 100")
    assert solved == good and len(solved) >= 2
    # a size no part reaches: no part, every slot unused
    none = cloud_twists(cloud, keys=keys, min_nodes=int(sizes.max()) + 1)
    assert int(none.count.item()) == 0 and (none.labels == -1).all() and not none.row_residual.any()
    for f in FIELDS[2:-1]:
        assert not getattr(none, f).any(), f
