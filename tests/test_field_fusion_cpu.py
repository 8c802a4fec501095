"""Host-side tests of the multi-view fusion (field_volume.fuse_views and the ``views_per_scene`` keyword of extract_field /
extract_mesh; njf_field_fuse / njf_field_combine): properties of the numpy restatement of the semantics
(tests/field_fusion_restatement.py), every argument check -- raised before any device work: there is no GPU here -- and the
C ABI's symbols and constants."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import field_fusion_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSION_SYMBOLS = ("njf_field_fuse", "njf_field_combine")
E_NULL, E_SHAPE, E_ACTION_DIM, E_VALUE = -1, -2, -3, -8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


def _case(g=2, v=3, n=257, seed=0):
    rng = np.random.default_rng(seed)
    values = rng.gamma(2.0, 1.0, size=(g, v, n)).astype(np.float32)
    seen = rng.random((g, v, n)) < 0.6
    seen[:, :, :5] = False                      # c = 0
    seen[:, :, 5:10] = True                     # c = V
    return values, seen


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_a_single_view_is_the_identity_on_seen_nodes(mode):
    values, seen = _case(v=1)
    fused, mask, valid = R.fuse(values, seen, mode, 1)
    assert fused.dtype == np.float32 and mask.dtype == np.uint8 and valid.dtype == bool
    assert np.array_equal(valid, seen[:, 0]) and np.array_equal(mask, seen[:, 0].astype(np.uint8))
    assert np.array_equal(fused[valid], values[:, 0][valid]) and (fused[~valid] == 0).all()


def test_min_mean_max_are_ordered_and_agree_with_a_plain_evaluation():
    values, seen = _case()
    lo, mask, valid = R.fuse(values, seen, "min", 1)
    mean, mask2, valid2 = R.fuse(values, seen, "mean", 1)
    hi, _, _ = R.fuse(values, seen, "max", 1)
    assert np.array_equal(mask, mask2) and np.array_equal(valid, valid2) and valid.any() and (~valid).any()
    # (the fp32 mean of numbers in [lo, hi] may leave the interval by its rounding only: one ulp per add and the division)
    slack = 4 * np.spacing(hi)
    assert (lo[valid] <= mean[valid] + slack[valid]).all() and (mean[valid] <= hi[valid] + slack[valid]).all()
    masked = np.where(seen, values.astype(np.float64), np.nan)
    count = seen.sum(axis=1)
    assert np.array_equal(valid, count >= 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (the all-NaN columns of the nodes nobody sees)
        assert np.array_equal(lo[valid], np.nanmin(masked, axis=1)[valid].astype(np.float32))
        assert np.array_equal(hi[valid], np.nanmax(masked, axis=1)[valid].astype(np.float32))
        assert np.allclose(mean[valid], (np.nansum(masked, axis=1) / count)[valid], rtol=1e-6, atol=0)
    for k in range(values.shape[1]):
        assert np.array_equal((mask >> k) & 1, seen[:, k].astype(np.uint8))


@pytest.mark.parametrize("mode", ["min", "max"])
def test_min_and_max_do_not_depend_on_the_order_of_the_views(mode):
    values, seen = _case()
    fused, _, valid = R.fuse(values, seen, mode, 2)
    for perm in ((2, 0, 1), (1, 0, 2), (2, 1, 0)):
        again, _, valid_again = R.fuse(values[:, perm], seen[:, perm], mode, 2)
        assert np.array_equal(fused, again) and np.array_equal(valid, valid_again)


@pytest.mark.parametrize("mode", R.MODES)
def test_min_views_masks_nodes_that_too_few_views_see(mode):
    values, seen = _case()
    count = seen.sum(axis=1)
    previous = None
    for min_views in (1, 2, 3):
        fused, mask, valid = R.fuse(values, seen, mode, min_views)
        assert np.array_equal(valid, count >= min_views)
        assert (fused[~valid] == 0).all() and (fused[valid] > 0).all()
        if previous is not None:                     # a stricter mask removes nodes and changes nothing else
            assert np.array_equal(fused[valid], previous[0][valid]) and np.array_equal(mask, previous[1])
        previous = (fused, mask)
    assert (count == 0).any() and (count == 3).any() and ((count > 0) & (count < 3)).any()


def test_the_combination_is_a_weighted_mean_with_the_stated_fallback():
    rng = np.random.default_rng(3)
    density = rng.gamma(2.0, 1.0, size=(40, 3)).astype(np.float32)
    seen = rng.random((40, 3)) < 0.6
    seen[0] = False                                  # nobody sees the position: the plain mean
    density[1] = 0.0                                 # every density is zero: the plain mean
    seen[1] = True
    seen[2] = (True, False, False)                   # one view: that view's row
    rows = rng.normal(size=(40, 3, 5)).astype(np.float32)
    out = R.combine(density, seen, rows)
    assert out.dtype == np.float64
    assert np.allclose(out[0], rows[0].astype(np.float64).mean(axis=0)) and np.allclose(out[1], rows[1].astype(np.float64).mean(axis=0))
    assert np.allclose(out[2], rows[2, 0], rtol=1e-7)
    w, total = R.weights(density, seen)
    assert w.dtype == np.float32 and total.dtype == np.float32 and (total > 0).all()
    assert (out >= rows.min(axis=1) - 1e-6).all() and (out <= rows.max(axis=1) + 1e-6).all()     # a convex combination
    assert np.array_equal(R.views_mask(seen)[:3], np.array([0, 7, 1], dtype=np.uint8))
    assert np.array_equal(R.combine_bound(rows), 2 * 8 * 2.0 ** -24 * np.abs(rows).max(axis=1))


# ---- argument checks, before any device work --------------------------------------------------------------------------------------
def _grid(dims=(4, 3, 5)):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds((0, 0, 1), (1, 1, 2), dims)


def test_fuse_views_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, fuse_views
    grid = _grid()
    values = torch.zeros(6, grid.num_nodes)
    for wrong in (values[0], values[:, :-1], values.double(), values.reshape(6, 4, 3, 5), values.numpy()):
        with pytest.raises(ValueError, match="values must be"):
            fuse_views(grid, wrong, views_per_scene=2)
    with pytest.raises(ValueError, match="does not divide"):
        fuse_views(grid, values, views_per_scene=4)
    with pytest.raises(ValueError, match="at most 8"):
        fuse_views(grid, torch.zeros(9, grid.num_nodes), views_per_scene=9)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="views_per_scene must be"):
            fuse_views(grid, values, views_per_scene=bad)
    for bad in ("median", "MEAN", None, 0):
        with pytest.raises(ValueError, match="fuse must be one of"):
            fuse_views(grid, values, views_per_scene=2, mode=bad)
    for bad in (0, 3, -1, 1.0, None):
        with pytest.raises(ValueError, match="min_views must be"):
            fuse_views(grid, values, views_per_scene=2, min_views=bad)
    big = FieldGrid((0, 0, 0), (1, 1, 1), (1024, 1024, 64))            # 2**26 nodes: 32 batch elements reach 2**31
    with pytest.raises(ValueError, match=r"2\*\*31"):
        fuse_views(big, torch.empty(32, big.num_nodes, device="meta"), views_per_scene=4)
    with pytest.raises(ValueError, match="no CPU path"):                # every check passed: there is nothing behind them
        fuse_views(grid, values, views_per_scene=3, mode="min", min_views=3)


@pytest.fixture(scope="module")
def host_model():
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model
    return Model(model_cfg_from_dict({"action_dim": 4, "action_decoder": {"name": "jacobian_mlp"}}))


def _encoding(batch):
    from neural_jacobian_field_amd.decoder import PixelEncoding
    return PixelEncoding(features=torch.zeros(batch, 512, 4, 4), extrinsics=torch.eye(4)[None].repeat(batch, 1, 1),
                         intrinsics=torch.eye(3)[None].repeat(batch, 1, 1), action=None)


@pytest.mark.parametrize("which", ["extract_field", "extract_mesh"])
def test_the_extractions_check_the_fusion_keywords_before_any_gpu_work(host_model, which):
    from neural_jacobian_field_amd import field_volume
    extract = getattr(field_volume, which)
    grid = _grid()
    with pytest.raises(ValueError, match="does not divide"):
        extract(host_model, _encoding(3), grid, 1.0, views_per_scene=2)
    with pytest.raises(ValueError, match="at most 8"):
        extract(host_model, _encoding(9), grid, 1.0, views_per_scene=9)
    with pytest.raises(ValueError, match="views_per_scene must be"):
        extract(host_model, _encoding(2), grid, 1.0, views_per_scene=0)
    with pytest.raises(ValueError, match="fuse must be one of"):
        extract(host_model, _encoding(2), grid, 1.0, views_per_scene=2, fuse="median")
    for bad in (0, 3):
        with pytest.raises(ValueError, match="min_views must be"):
            extract(host_model, _encoding(2), grid, 1.0, views_per_scene=2, min_views=bad)
    with pytest.raises(ValueError, match="GPU"):                        # and there is no CPU path behind the checks
        extract(host_model, _encoding(2), grid, 1.0, views_per_scene=2, fuse="min", min_views=2)


def test_a_proposal_cull_is_refused_for_fused_scenes(host_model):
    from neural_jacobian_field_amd.field_volume import extract_field
    with pytest.raises(ValueError, match="cull"):
        extract_field(host_model, _encoding(2), _grid(), 1.0, cull=0.5, views_per_scene=2)
    with pytest.raises(ValueError, match="GPU"):                        # a single view keeps its cull
        extract_field(host_model, _encoding(2), _grid(), 1.0, cull=0.5, views_per_scene=1)


def test_the_model_passes_the_keywords_through():
    import inspect
    from neural_jacobian_field_amd.field_volume import FieldMesh, FieldPointCloud
    from neural_jacobian_field_amd.model import Model
    for fn in (Model.extract_field, Model.extract_mesh):
        params = inspect.signature(fn).parameters
        assert params["views_per_scene"].default == 1 and params["fuse"].default == "mean" and params["min_views"].default == 1
    assert list(FieldPointCloud.__dataclass_fields__)[-1] == "views" and FieldPointCloud.__dataclass_fields__["views"].default is None
    assert list(FieldMesh.__dataclass_fields__)[-1] == "vertex_views"
    assert FieldMesh.__dataclass_fields__["vertex_views"].default is None


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_fusion_symbols_are_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    for name in FUSION_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/njf_hip.h"
        assert name in hip.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.njf_abi_version() == 20          # the change is additive
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in FUSION_SYMBOLS:                 # the bound signatures have the header's number of parameters
        params = re.search(name + r"\s*\((.*?)\);", flat, flags=re.S).group(1)
        assert len(params.split(",")) == len(getattr(lib, name).argtypes), name


def test_both_tables_of_constants_agree_with_the_header():
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", header).group(1))

    assert define("NJF_FIELD_MAX_VIEWS") == hip.FIELD_MAX_VIEWS == 8
    modes = {"mean": define("NJF_FIELD_FUSE_MEAN"), "min": define("NJF_FIELD_FUSE_MIN"), "max": define("NJF_FIELD_FUSE_MAX")}
    assert modes == hip.FIELD_FUSE_MODES and len(set(modes.values())) == 3
    assert (hip.FIELD_FUSE_MEAN, hip.FIELD_FUSE_MIN, hip.FIELD_FUSE_MAX) == (modes["mean"], modes["min"], modes["max"])
    assert tuple(sorted(hip.FIELD_FUSE_MODES)) == tuple(sorted(R.MODES))


def test_the_c_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks (or has nothing to do)
    grid = hip.make_field_grid((0.0, 0.0, 1.0), (0.1, 0.1, 0.1), (4, 5, 6))

    def fuse(g=grid, cams=None, scenes=2, views=3, values=P, mode=0, min_views=1, fused=P):
        return lib.njf_field_fuse(C.byref(g), None if cams is None else C.byref(cams), scenes, views, values, mode, min_views,
                                  fused, None, None, None)

    assert fuse(views=0) == E_VALUE and fuse(views=9) == E_VALUE
    assert fuse(min_views=0) == E_VALUE and fuse(min_views=4) == E_VALUE
    assert fuse(mode=3) == E_VALUE and fuse(mode=-1) == E_VALUE
    assert fuse(values=None) == E_NULL and fuse(fused=None) == E_NULL
    assert fuse(scenes=0) == E_SHAPE
    assert fuse(g=hip.make_field_grid((0, 0, 0), (1, 1, 1), (1024, 1024, 512)), scenes=1, views=4) == E_SHAPE   # G*V*N = 2^31
    assert fuse(cams=hip.Cameras(P, P, None, None, None, None, None, 5, 0)) == E_SHAPE                           # batch != G*V
    assert fuse(cams=hip.Cameras(P, None, None, None, None, None, None, 6, 0)) == E_NULL

    def combine(capacity=8, nodes=120, views=3, cams=None, density=P, color=P, jacobian=P, a_dim=4, out_color=P, out_jacobian=P,
                out_views=P):
        return lib.njf_field_combine(P, P, None, capacity, nodes, views, None if cams is None else C.byref(cams), density, color,
                                     jacobian, a_dim, out_color, out_jacobian, out_views, None)

    assert combine(views=0) == E_VALUE and combine(views=9) == E_VALUE and combine(nodes=0) == E_VALUE
    assert combine(capacity=-1) == E_SHAPE
    assert combine(density=None) == E_NULL and combine(out_color=None) == E_NULL and combine(out_jacobian=None) == E_NULL
    assert combine(color=None, jacobian=None, out_views=None) == E_NULL
    assert combine(a_dim=0) == E_ACTION_DIM and combine(a_dim=11) == E_ACTION_DIM
    assert combine(cams=hip.Cameras(P, P, None, None, None, None, None, 4, 0)) == E_SHAPE                        # 4 cameras, 3 views
    assert combine(capacity=0) == 0                                                                              # nothing launched
