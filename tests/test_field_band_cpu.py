"""Host-side tests of the coarse-to-fine band (field_volume.band_from_values / band_leaks, the ``coarse`` keywords of
extract_field / extract_mesh; njf_field_band / njf_field_scatter / njf_field_band_leaks): the numpy
restatement (tests/field_band_restatement.py) against a brute-force triple loop, the coordinate identity coarse node j = fine
node k*j, every argument check -- raised before any device work: there is no GPU here -- and the C ABI's symbols."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import field_band_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"njf_field_band": 14, "njf_field_scatter": 7, "njf_field_band_leaks": 8}
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


def _grid(dims=(9, 13, 17)):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), dims)


# ---- the restatement against a brute-force loop ------------------------------------------------------------------------------------
def _brute(values, valid, threshold, dims, k, d):
    """Section 14 word by word, one node at a time."""
    m = tuple((n - 1) // k for n in dims)
    batch = values.shape[0]
    coarse = values.reshape((batch,) + tuple(mc + 1 for mc in m))
    cvalid = None if valid is None else valid.reshape(coarse.shape)
    active = np.zeros((batch,) + m, dtype=bool)
    for b, jx, jy, jz in itertools.product(range(batch), range(m[0]), range(m[1]), range(m[2])):
        for qx in range(max(0, jx - d), min(m[0], jx + 1 + d) + 1):
            for qy in range(max(0, jy - d), min(m[1], jy + 1 + d) + 1):
                for qz in range(max(0, jz - d), min(m[2], jz + 1 + d) + 1):
                    v = coarse[b, qx, qy, qz]
                    if (cvalid is None or cvalid[b, qx, qy, qz]) and not np.isnan(v) and v >= np.float32(threshold):
                        active[b, jx, jy, jz] = True
    band = np.zeros((batch,) + tuple(dims), dtype=bool)
    for b, ix, iy, iz in itertools.product(range(batch), range(dims[0]), range(dims[1]), range(dims[2])):
        cand = [sorted({-(-i // k) - 1, i // k} & set(range(mc))) for i, mc in zip((ix, iy, iz), m)]
        band[b, ix, iy, iz] = any(active[b, jx, jy, jz] for jx in cand[0] for jy in cand[1] for jz in cand[2])
    return active.reshape(batch, -1), band.reshape(batch, -1)


def _brute_leaks(inside, band, dims):
    batch = inside.shape[0]
    ins, bnd = inside.reshape((batch,) + tuple(dims)), band.reshape((batch,) + tuple(dims))
    count = 0
    for b, ix, iy, iz in itertools.product(range(batch), range(dims[0]), range(dims[1]), range(dims[2])):
        if not ins[b, ix, iy, iz]:
            continue
        leak = False
        for (dx, dy, dz), sign in itertools.product(R.DIRECTIONS, (1, -1)):
            x, y, z = ix + sign * dx, iy + sign * dy, iz + sign * dz
            if 0 <= x < dims[0] and 0 <= y < dims[1] and 0 <= z < dims[2] and not bnd[b, x, y, z]:
                leak = True
        count += leak
    return count


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_the_restatement_equals_a_brute_force_loop(k, d):
    dims, batch = (5, 9, 5), 2
    m = R.blocks_per_axis(dims, k)
    coarse_nodes = (m[0] + 1) * (m[1] + 1) * (m[2] + 1)
    rng = np.random.default_rng(10 * k + d)
    values = rng.random((batch, coarse_nodes)).astype(np.float32)
    values[0, 1] = np.nan
    values[1, 2] = np.inf
    valid = rng.random(values.shape) < 0.7
    for threshold, mask in ((0.9, None), (0.8, valid), (0.5, valid), (2.0, None), (-1.0, None)):
        active, band, index, count = R.full(values, mask, threshold, dims, k, d)
        ref_active, ref_band = _brute(values, mask, threshold, dims, k, d)
        assert np.array_equal(active, ref_active) and np.array_equal(band, ref_band), (threshold, mask is None)
        assert count == ref_band.sum() and np.array_equal(index, np.flatnonzero(ref_band.reshape(-1)))
        inside = band & (rng.random(band.shape) < 0.5)
        assert R.leaks(inside, band, dims) == _brute_leaks(inside, band, dims)
    assert R.full(values, None, 2.0, dims, k, d)[3] > 0                      # +inf is a hit
    assert R.full(np.nan_to_num(values, posinf=0.0), None, 2.0, dims, k, d)[3] == 0       # nothing hits: the empty band
    assert R.full(values, None, -1.0, dims, k, 2)[1].sum() > 0


def test_the_restatement_on_hand_cases():
    dims, k = (5, 5, 9), 4                                                     # m = (1, 1, 2): two blocks along z
    hit = np.zeros((1, 2 * 2 * 3), dtype=bool)
    hit[0, 0] = True                                                          # coarse node (0, 0, 0): a corner of block 0 only
    assert R.blocks(hit, dims, k, 0).tolist() == [[True, False]]
    assert R.blocks(hit, dims, k, 1).tolist() == [[True, True]]               # one coarse node further: block 1
    band = R.band(np.array([[True, False]]), dims, k).reshape(dims)
    assert band[:, :, :5].all() and not band[:, :, 5:].any()                  # the shared face z = 4 belongs to the active block
    assert R.leaks(band.reshape(1, -1), band.reshape(1, -1), dims) == 25      # the nodes of that face look out of the band
    inner = band.copy()
    inner[:, :, 4] = False
    assert R.leaks(inner.reshape(1, -1), band.reshape(1, -1), dims) == 0


# ---- coarse node j IS fine node k*j -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_a_coarse_node_has_the_coordinates_of_fine_node_k_j(k):
    from neural_jacobian_field_amd.field_volume import FieldGrid, coarse_grid
    dims = (2 * k + 1, k + 1, 3 * k + 1)
    for fine in (_grid(dims), FieldGrid((0.1, -0.3, 1e-3), (1.0 / 3.0, 0.017, 1e-7), dims)):
        coarse = coarse_grid(fine, k)
        assert coarse.dims == (3, 2, 4) and coarse.origin == fine.origin
        assert coarse.step == tuple(k * s for s in fine.step)                # exact: a power of two
        j = np.stack(np.meshgrid(*[np.arange(n) for n in coarse.dims], indexing="ij"), axis=-1).reshape(-1, 3)
        at = torch.from_numpy(fine.linear_index(k * j[:, 0], k * j[:, 1], k * j[:, 2]))
        assert torch.equal(coarse.points(), fine.points(at))                 # bit for bit


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def test_band_from_values_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import band_from_values
    grid = _grid()                                                            # (9, 13, 17): k = 4 gives 3 * 4 * 5 coarse nodes
    values = torch.zeros(2, 60)
    for bad in (0, 1, 3, 6, 32, True, 4.0, None):
        with pytest.raises(ValueError, match="coarse factor"):
            band_from_values(grid, bad, values, 0.5)
    with pytest.raises(ValueError, match="on every axis"):
        band_from_values(grid, 8, values, 0.5)                                # 13 - 1 is no multiple of 8
    with pytest.raises(ValueError, match="on every axis"):
        band_from_values(_grid((9, 9, 9)), 16, values, 0.5)                   # n < k + 1
    for bad in (-1, 3, 1.0, True, None):
        with pytest.raises(ValueError, match="coarse_dilate"):
            band_from_values(grid, 4, values, 0.5, dilate=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            band_from_values(grid, 4, values, bad)
    for bad in (torch.zeros(2, 61), torch.zeros(60), torch.zeros(2, 60, dtype=torch.float64), np.zeros((2, 60), dtype=np.float32)):
        with pytest.raises(ValueError, match="coarse_values must be fp32"):
            band_from_values(grid, 4, bad, 0.5)
    for bad in (torch.ones(2, 59, dtype=torch.bool), torch.ones(2, 60)):
        with pytest.raises(ValueError, match="coarse_valid must be"):
            band_from_values(grid, 4, values, 0.5, coarse_valid=bad)
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError, match="max_nodes"):
            band_from_values(grid, 4, values, 0.5, max_nodes=bad)
    with pytest.raises(ValueError, match="no CPU path"):
        band_from_values(grid, 4, values, 0.5)


def test_band_leaks_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import band_leaks
    grid = _grid((5, 5, 5))
    band, index = torch.ones(2, 125, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)
    for bad in (torch.ones(2, 124, dtype=torch.uint8), torch.ones(250, dtype=torch.uint8), torch.ones(2, 125)):
        with pytest.raises(ValueError, match="band must be"):
            band_leaks(grid, bad, index)
    for bad in (index.long(), index.reshape(1, 3)):
        with pytest.raises(ValueError, match="index must be int32"):
            band_leaks(grid, band, bad)
    with pytest.raises(ValueError, match="count must be one int32"):
        band_leaks(grid, band, index, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU path"):
        band_leaks(grid, band, index)


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
@pytest.mark.parametrize("views", [1, 2])
def test_the_extractions_check_the_band_keywords_before_any_gpu_work(host_model, which, views):
    from neural_jacobian_field_amd import field_volume
    extract = getattr(field_volume, which)
    grid, kw = _grid(), dict(views_per_scene=views)
    for bad in (0, 3, 5, 32, True, 2.0):
        with pytest.raises(ValueError, match="coarse factor"):
            extract(host_model, _encoding(2), grid, 1.0, coarse=bad, **kw)
    with pytest.raises(ValueError, match="on every axis"):
        extract(host_model, _encoding(2), grid, 1.0, coarse=8, **kw)
    for bad in (-1, 3, 1.5, True):
        with pytest.raises(ValueError, match="coarse_dilate"):
            extract(host_model, _encoding(2), grid, 1.0, coarse=4, coarse_dilate=bad, **kw)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="coarse_threshold must be finite"):
            extract(host_model, _encoding(2), grid, 1.0, coarse=4, coarse_threshold=bad, **kw)
    with pytest.raises(ValueError, match="without coarse"):
        extract(host_model, _encoding(2), grid, 1.0, coarse_threshold=0.5, **kw)
    with pytest.raises(ValueError, match="GPU"):                               # and there is no CPU path behind the checks
        extract(host_model, _encoding(2), grid, 1.0, coarse=4, coarse_threshold=0.5, coarse_dilate=2, **kw)


def test_the_signatures_carry_the_new_defaults():
    from neural_jacobian_field_amd import field_volume
    from neural_jacobian_field_amd.model import Model
    for fn in (Model.extract_field, field_volume.extract_field, Model.extract_mesh, field_volume.extract_mesh):
        params = inspect.signature(fn).parameters
        assert params["coarse"].default is None and params["coarse_threshold"].default is None
        assert params["coarse_dilate"].default == 1 and params["coarse"].kind is inspect.Parameter.KEYWORD_ONLY
    params = inspect.signature(field_volume.band_from_values).parameters
    assert [params[k].default for k in ("coarse_valid", "dilate", "max_nodes")] == [None, 1, None]
    assert inspect.signature(field_volume.band_leaks).parameters["count"].default is None
    assert list(field_volume.FieldBand.__dataclass_fields__) == ["coarse_grid", "block_active", "band", "index", "count"]
    # the result classes keep their fields: band_count and band_leaks are attributes, set like components_status
    assert list(field_volume.FieldPointCloud.__dataclass_fields__)[-1] == "views"
    assert list(field_volume.FieldMesh.__dataclass_fields__)[-1] == "vertex_views"


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for symbol, arguments in SYMBOLS.items():
        assert symbol in declared, f"{symbol} is not declared in include/njf_hip.h"
        assert symbol in hip.EXPORTED_SYMBOLS
        assert hasattr(lib, symbol), f"{symbol} is not exported by the library"
        params = re.search(symbol + r"\s*\((.*?)\);", flat, flags=re.S).group(1)
        assert len(params.split(",")) == len(getattr(lib, symbol).argtypes) == arguments
    assert lib.njf_abi_version() == 20          # the change is additive
    block = int(re.search(r"#define NJF_FIELD_BAND_BLOCK (\d+)", header).group(1))
    assert block == hip.FIELD_BAND_BLOCK == hip.FIELD_SELECT_BLOCK == 1024
    assert hip.FIELD_BAND_FACTORS == R.FACTORS == (2, 4, 8, 16) and hip.FIELD_BAND_MAX_DILATE == 2


def test_the_c_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    grid = hip.make_field_grid((0.0, 0.0, 1.0), (0.1, 0.1, 0.1), (9, 13, 17))

    def band(g=grid, factor=4, dilate=1, batch=2, values=P, valid=None, threshold=0.5, active=P, out=P, indices=P, count=P,
             capacity=10, workspace=P):
        return lib.njf_field_band(None if g is None else C.byref(g), factor, dilate, batch, values, valid, threshold, active, out,
                                  indices, count, capacity, workspace, None)

    for bad in (0, 1, 3, 6, 12, 32, -4):
        assert band(factor=bad) == E_VALUE
    assert band(factor=8) == E_VALUE                                            # 13 - 1 is no multiple of 8
    assert band(g=hip.make_field_grid((0, 0, 0), (1, 1, 1), (9, 9, 9)), factor=16) == E_VALUE      # n < k + 1
    assert band(g=hip.make_field_grid((0, 0, 0), (1, 1, 1), (9, 10, 9))) == E_VALUE
    for bad in (-1, 3):
        assert band(dilate=bad) == E_VALUE
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert band(threshold=bad) == E_VALUE
    assert band(g=None) == E_NULL
    for missing in ("values", "active", "out", "count", "workspace", "indices"):
        assert band(**{missing: None}) == E_NULL, missing
    assert band(capacity=-1) == E_SHAPE
    assert band(batch=0) == E_SHAPE
    assert band(g=hip.make_field_grid((0, 0, 0), (1, 1, 1), (1025, 1025, 513)), batch=4) == E_SHAPE        # B*N >= 2^31

    def scatter(values=P, indices=P, count=None, capacity=5, out=P, out_size=10):
        return lib.njf_field_scatter(values, indices, count, capacity, out, out_size, None)

    assert scatter(capacity=-1) == E_SHAPE and scatter(out_size=-1) == E_SHAPE
    for missing in ("values", "indices", "out"):
        assert scatter(**{missing: None}) == E_NULL, missing
    assert scatter(capacity=0, values=None, indices=None) == 0                  # nothing to do: no launch

    def leaks(g=grid, batch=2, out=P, indices=P, count=None, capacity=5, n=P):
        return lib.njf_field_band_leaks(None if g is None else C.byref(g), batch, out, indices, count, capacity, n, None)

    assert leaks(g=None) == E_NULL
    for missing in ("out", "indices", "n"):
        assert leaks(**{missing: None}) == E_NULL, missing
    assert leaks(capacity=-1) == E_SHAPE and leaks(batch=0) == E_SHAPE
    assert leaks(g=hip.make_field_grid((0, 0, 0), (1, 1, 1), (1024, 1024, 512)), batch=4) == E_SHAPE


def test_the_wrappers_refuse_cpu_tensors_and_wrong_sizes():
    from neural_jacobian_field_amd import hip
    grid = hip.make_field_grid((0.0, 0.0, 1.0), (0.1, 0.1, 0.1), (5, 5, 5))
    u8, i32 = dict(dtype=torch.uint8), dict(dtype=torch.int32)
    args = dict(coarse_values=torch.zeros(16), coarse_threshold=0.5, block_active=torch.zeros(2, **u8),
                band=torch.zeros(250, **u8), out_indices=torch.zeros(250, **i32), out_count=torch.zeros(1, **i32))
    with pytest.raises(ValueError, match="must live on the GPU"):
        hip.field_band(grid, 4, 1, 2, **args)
    with pytest.raises(ValueError, match="block_active must hold 16"):
        hip.field_band(grid, 2, 1, 2, **dict(args, coarse_values=torch.zeros(54)))
    with pytest.raises(ValueError, match="must live on the GPU"):
        hip.field_scatter(torch.zeros(4), torch.zeros(4, **i32), None, 4, torch.zeros(10))
    with pytest.raises(ValueError, match="shorter than the capacity"):
        hip.field_scatter(torch.zeros(3), torch.zeros(4, **i32), None, 4, torch.zeros(10))
    with pytest.raises(ValueError, match="must live on the GPU"):
        hip.field_band_leaks(grid, 2, torch.zeros(250, **u8), torch.zeros(4, **i32), None, 4, torch.zeros(1, **i32))
