"""Host-side tests of the connected-component labelling (field_volume.label_components / cloud_components / dominant_joint,
the ``min_component_nodes`` / ``largest_only`` keywords of extract_field / extract_mesh; njf_field_components; DESIGN.md
section 13): the numpy restatement of the semantics (tests/field_components_restatement.py) against ``scipy.ndimage.label``,
every argument check -- raised before any device work: there is no GPU here --, ``keep`` and ``dominant_joint`` on CPU tensors,
and the C ABI's symbol and constants."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_components_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "njf_field_components"
E_NULL, E_SHAPE, E_VALUE = -1, -2, -8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("occupancy", [0.15, 0.3, 0.6])
def test_the_restatement_agrees_with_scipy(connectivity, occupancy):
    from scipy import ndimage
    dims, batch = (7, 9, 8), 3
    nodes = dims[0] * dims[1] * dims[2]
    inside = np.random.default_rng(int(100 * occupancy) + connectivity).random((batch, nodes)) < occupancy
    labels, sizes, count = R.label(inside, dims, connectivity)
    total = 0
    for b in range(batch):                                    # one batch element at a time: nothing joins two of them
        lab, n = ndimage.label(inside[b].reshape(dims), structure=R.structure(connectivity))
        lab = lab.reshape(-1)
        total += n
        expect_labels = np.full(nodes, -1, dtype=np.int64)
        expect_sizes = np.zeros(nodes, dtype=np.int64)
        for c in range(1, n + 1):                             # relabel to the minimum global index
            members = np.flatnonzero(lab == c)
            expect_labels[members] = b * nodes + members.min()
            expect_sizes[members] = members.size
        assert np.array_equal(labels[b], expect_labels) and np.array_equal(sizes[b], expect_sizes)
    assert count == total == int((labels == np.arange(batch * nodes).reshape(batch, nodes)).sum()) and count > 1
    assert labels.dtype == np.int32 and sizes.dtype == np.int32
    # and FieldComponents.keep (integer torch ops, here on CPU tensors) selects what the restatement selects
    comp = _components(labels.tolist(), sizes.tolist())
    for min_nodes, largest_only in ((1, False), (3, False), (int(sizes.max()), False), (1, True), (int(sizes.max()) + 1, True)):
        assert np.array_equal(comp.keep(min_nodes, largest_only).numpy(), R.keep(labels, sizes, min_nodes, largest_only))


def test_the_restatement_on_hand_cases():
    dims = (3, 3, 3)

    def at(*nodes):
        inside = np.zeros((1, 27), dtype=bool)
        for ix, iy, iz in nodes:
            inside[0, (ix * 3 + iy) * 3 + iz] = True
        return inside

    assert R.label(at((0, 0, 0), (1, 1, 0)), dims, 6)[2] == 2 and R.label(at((0, 0, 0), (1, 1, 0)), dims, 14)[2] == 1
    assert R.label(at((1, 0, 0), (0, 1, 0)), dims, 6)[2] == 2 and R.label(at((1, 0, 0), (0, 1, 0)), dims, 14)[2] == 2  # anti-diagonal
    assert R.label(at((0, 0, 2), (0, 1, 0)), dims, 14)[2] == 2                  # linear neighbours n, n + 1: no wrap
    assert R.label(at((0, 0, 0), (1, 1, 1)), dims, 14)[2] == 1 and R.label(at((0, 0, 0), (1, 1, 1)), dims, 6)[2] == 2
    inside = np.ones((2, 27), dtype=bool)
    labels, sizes, count = R.label(inside, dims, 6)
    assert count == 2 and (labels[0] == 0).all() and (labels[1] == 27).all() and (sizes == 27).all()
    keys = (np.indices(dims).sum(axis=0) % 2).reshape(1, 27)
    labels, sizes, count = R.label(inside[:1], dims, 6, keys)                   # checkerboard keys: nothing joins along an axis
    assert count == 27 and (sizes == 1).all() and np.array_equal(labels[0], np.arange(27))
    assert R.label(inside[:1], dims, 6, np.zeros((1, 27), dtype=np.int32))[2] == 1
    assert len(R.offsets(6)) == 6 and len(R.offsets(14)) == 14 and (1, -1, 0) not in R.offsets(14)
    # the direction table is section 11's, the connectivities are the library's
    from neural_jacobian_field_amd import field_volume, hip
    assert R.DIRECTIONS == field_volume.MESH_DIRECTIONS and R.CONNECTIVITIES == hip.FIELD_COMPONENTS_CONNECTIVITIES


# ---- keep and dominant_joint on the CPU tensors they accept --------------------------------------------------------------------------
def _components(labels, sizes):
    from neural_jacobian_field_amd.field_volume import FieldComponents, FieldGrid
    labels, sizes = torch.tensor(labels, dtype=torch.int32), torch.tensor(sizes, dtype=torch.int32)
    grid = FieldGrid((0, 0, 0), (1, 1, 1), (1, 1, labels.shape[1]))
    return FieldComponents(grid=grid, labels=labels, sizes=sizes, count=torch.zeros(1, dtype=torch.int32),
                           status=torch.zeros(1, dtype=torch.int32))


def test_keep_on_hand_cases():
    # element 0: components {0,1} (2 nodes), {3} (1), {5,6} (2: a size tie with the first); element 1: nothing inside but node 8+2
    comp = _components([[0, 0, -1, 3, -1, 5, 5, -1], [-1, -1, 10, -1, -1, -1, -1, -1]],
                       [[2, 2, 0, 1, 0, 2, 2, 0], [0, 0, 1, 0, 0, 0, 0, 0]])
    t, f = True, False
    assert comp.keep().tolist() == [[t, t, f, t, f, t, t, f], [f, f, t, f, f, f, f, f]]
    assert comp.keep(2).tolist() == [[t, t, f, f, f, t, t, f], [f] * 8]
    assert comp.keep(3).tolist() == [[f] * 8, [f] * 8]
    assert comp.keep(largest_only=True).tolist() == [[t, t, f, f, f, f, f, f], [f, f, t, f, f, f, f, f]]      # the tie: smallest label
    assert comp.keep(2, largest_only=True).tolist() == [[t, t, f, f, f, f, f, f], [f] * 8]
    assert comp.keep().dtype == torch.bool
    empty = _components([[-1, -1, -1]], [[0, 0, 0]])
    assert not empty.keep(largest_only=True).any()
    for bad in (0, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="min_nodes"):
            comp.keep(bad)
    labels = np.array([[0, 0, -1, 3, -1, 5, 5, -1]], dtype=np.int32)
    sizes = np.array([[2, 2, 0, 1, 0, 2, 2, 0]], dtype=np.int32)
    for k, only in ((1, False), (2, False), (1, True), (3, True)):                     # and the restatement says the same
        assert np.array_equal(R.keep(labels, sizes, k, only), _components(labels.tolist(), sizes.tolist()).keep(k, only).numpy())


def test_dominant_joint_on_hand_cases():
    from neural_jacobian_field_amd.field_volume import dominant_joint
    jac = torch.tensor([[[1.0, 0, 0], [0, 2, 0], [0, 0, 1.5]],        # joint 1
                        [[0, 3, 4], [5, 0, 0], [0, 0, 0]],            # norms 5, 5, 0: the tie goes to joint 0
                        [[0, 0, 0], [0, 0, 0], [0, 0, 0]],            # all zero: joint 0
                        [[0, 0, -1], [0, 0, 0], [-2, 0, 0]]])         # signs do not matter: joint 2
    out = dominant_joint(jac)
    assert out.dtype == torch.int32 and out.tolist() == [1, 0, 0, 2]
    for wrong in (jac[0], jac[..., :2], jac.numpy(), torch.zeros(4, 0, 3)):
        with pytest.raises(ValueError, match=r"\[n, A, 3\]"):
            dominant_joint(wrong)


# ---- argument checks, before any device work --------------------------------------------------------------------------------------
def _grid(dims=(4, 3, 5)):
    from neural_jacobian_field_amd.field_volume import FieldGrid
    return FieldGrid.from_bounds((0, 0, 1), (1, 1, 2), dims)


def test_label_components_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldGrid, label_components
    grid = _grid()
    values = torch.zeros(2, grid.num_nodes)
    for wrong in (values[0], values[:, :-1], values.double(), values.numpy()):
        with pytest.raises(ValueError, match="values must be"):
            label_components(grid, wrong, 0.5)
    for bad in (0, 4, 8, 18, 26, 6.5, None, "6", True):
        with pytest.raises(ValueError, match="connectivity must be 6 or 14"):
            label_components(grid, values, 0.5, connectivity=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            label_components(grid, values, bad)
    keys = torch.zeros(2, grid.num_nodes, dtype=torch.int32)
    for wrong in (keys.long(), keys.float(), keys[0], keys[:, :-1], keys.numpy()):
        with pytest.raises(ValueError, match="keys must be int32"):
            label_components(grid, values, 0.5, keys=wrong)
    for wrong in (torch.ones(2, grid.num_nodes), torch.ones(grid.num_nodes, dtype=torch.bool)):
        with pytest.raises(ValueError, match="valid must be"):
            label_components(grid, values, 0.5, valid=wrong)
    big = FieldGrid((0, 0, 0), (1, 1, 1), (1024, 1024, 64))
    with pytest.raises(ValueError, match=r"2\*\*31"):
        label_components(big, torch.empty(32, big.num_nodes, device="meta"), 0.5)
    with pytest.raises(ValueError, match="no CPU path"):                # every check passed: there is nothing behind them
        label_components(grid, values, 0.5, connectivity=14, keys=keys, valid=torch.ones(2, grid.num_nodes, dtype=torch.bool))


def test_cloud_components_checks_its_arguments_before_any_gpu_work():
    from neural_jacobian_field_amd.field_volume import FieldPointCloud, cloud_components
    grid = _grid()
    n = 5
    cloud = FieldPointCloud(grid=grid, index=torch.arange(n, dtype=torch.int32), xyz=torch.zeros(n, 3), density=torch.zeros(n),
                            color=None, jacobian=None, count=torch.tensor([n], dtype=torch.int32))
    with pytest.raises(ValueError, match="connectivity must be 6 or 14"):
        cloud_components(cloud, connectivity=26)
    for wrong in (torch.zeros(n), torch.zeros(n + 1, dtype=torch.int32), torch.zeros(n, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="keys must be int32"):
            cloud_components(cloud, keys=wrong)
    with pytest.raises(ValueError, match="no CPU path"):
        cloud_components(cloud, keys=torch.zeros(n, dtype=torch.int32))


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
def test_the_extractions_check_the_component_keywords_before_any_gpu_work(host_model, which):
    from neural_jacobian_field_amd import field_volume
    extract = getattr(field_volume, which)
    grid = _grid()
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="min_component_nodes must be"):
            extract(host_model, _encoding(2), grid, 1.0, min_component_nodes=bad)
    if which == "extract_field":
        for bad in (0, 8, 26, None):
            with pytest.raises(ValueError, match="connectivity must be 6 or 14"):
                extract(host_model, _encoding(2), grid, 1.0, min_component_nodes=2, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity must be 6 or 14"):     # checked also when the filter is off
            extract(host_model, _encoding(2), grid, 1.0, connectivity=7)
    else:
        assert "connectivity" not in inspect.signature(extract).parameters         # 14 by construction
    with pytest.raises(ValueError, match="GPU"):                                   # and there is no CPU path behind the checks
        extract(host_model, _encoding(2), grid, 1.0, min_component_nodes=3, largest_only=True)


def test_the_signatures_carry_the_new_defaults():
    from neural_jacobian_field_amd import field_volume
    from neural_jacobian_field_amd.model import Model
    for fn in (Model.extract_field, field_volume.extract_field, Model.extract_mesh, field_volume.extract_mesh):
        params = inspect.signature(fn).parameters
        assert params["min_component_nodes"].default is None and params["largest_only"].default is False
        assert params["min_component_nodes"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (Model.extract_field, field_volume.extract_field):
        assert inspect.signature(fn).parameters["connectivity"].default == 6
    params = inspect.signature(field_volume.label_components).parameters
    assert [params[k].default for k in ("valid", "pixel_encoding", "connectivity", "keys")] == [None, None, 6, None]
    params = inspect.signature(field_volume.cloud_components).parameters
    assert params["connectivity"].default == 6 and params["keys"].default is None
    assert list(field_volume.FieldComponents.__dataclass_fields__) == ["grid", "labels", "sizes", "count", "status"]
    # the result classes keep their last field: per-row labels come from cloud_components
    assert list(field_volume.FieldPointCloud.__dataclass_fields__)[-1] == "views"
    assert list(field_volume.FieldMesh.__dataclass_fields__)[-1] == "vertex_views"


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    assert SYMBOL in declared, f"{SYMBOL} is not declared in include/njf_hip.h"
    assert SYMBOL in hip.EXPORTED_SYMBOLS
    assert hasattr(lib, SYMBOL), f"{SYMBOL} is not exported by the library"
    assert lib.njf_abi_version() == 20          # the change is additive
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    params = re.search(SYMBOL + r"\s*\((.*?)\);", flat, flags=re.S).group(1)
    assert len(params.split(",")) == len(getattr(lib, SYMBOL).argtypes) == 18


def test_the_constants_agree_with_the_header():
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", header).group(1))

    assert define("NJF_FIELD_COMPONENTS_BLOCK") == hip.FIELD_COMPONENTS_BLOCK == define("NJF_FIELD_SELECT_BLOCK") == 1024
    bits = (define("NJF_FIELD_COMPONENTS_E_LOCAL"), define("NJF_FIELD_COMPONENTS_E_FIND"), define("NJF_FIELD_COMPONENTS_E_UNION"))
    assert bits == (hip.FIELD_COMPONENTS_E_LOCAL, hip.FIELD_COMPONENTS_E_FIND, hip.FIELD_COMPONENTS_E_UNION) == (1, 2, 4)
    phases = tuple(define(f"NJF_FIELD_COMPONENTS_{n}") for n in ("INIT", "MERGE", "LABEL", "SIZES"))
    assert phases == hip.FIELD_COMPONENTS_PHASES == (1, 2, 4, 8) and define("NJF_FIELD_COMPONENTS_ALL") == hip.FIELD_COMPONENTS_ALL == 15
    assert hip.FIELD_COMPONENTS_CONNECTIVITIES == R.CONNECTIVITIES == (6, 14)


def test_the_c_entry_point_refuses_bad_arguments_without_a_gpu(lib):
    from neural_jacobian_field_amd import hip
    P = 0x1000                                   # never dereferenced: every call below fails its checks
    grid = hip.make_field_grid((0.0, 0.0, 1.0), (0.1, 0.1, 0.1), (4, 5, 6))

    def call(g=grid, cams=None, batch=2, values=P, valid=None, indices=None, count=None, capacity=0, keys=None, connectivity=6,
             phase=15, labels=P, sizes=P, n=P, status=P, workspace=P):
        return lib.njf_field_components(C.byref(g), None if cams is None else C.byref(cams), batch, values, 0.5, valid, indices,
                                        count, capacity, keys, connectivity, phase, labels, sizes, n, status, workspace, None)

    for bad in (0, 4, 8, 18, 26, -6):
        assert call(connectivity=bad) == E_VALUE
    for bad in (0, 16, -1):
        assert call(phase=bad) == E_VALUE
    assert call(values=None) == E_NULL                                       # neither form
    assert call(indices=P, capacity=3) == E_VALUE                            # both forms
    assert call(values=None, indices=P, capacity=3, valid=P) == E_VALUE      # a list is the inside set
    assert call(values=None, indices=P, capacity=3, cams=hip.Cameras(P, P, None, None, None, None, None, 2, 0)) == E_VALUE
    assert call(values=None, indices=P, capacity=-1) == E_SHAPE
    assert call(batch=0) == E_SHAPE
    assert call(g=hip.make_field_grid((0, 0, 0), (1, 1, 1), (4, 0, 6))) == E_SHAPE
    assert call(g=hip.make_field_grid((0, 0, 0), (1, 1, 1), (1024, 1024, 512)), batch=4) == E_SHAPE            # B*N = 2^31
    for missing in ("labels", "sizes", "n", "status", "workspace"):
        assert call(**{missing: None}) == E_NULL, missing
    assert call(cams=hip.Cameras(P, P, None, None, None, None, None, 3, 0)) == E_SHAPE                          # batch != B
    assert call(cams=hip.Cameras(P, None, None, None, None, None, None, 2, 0)) == E_NULL
