"""CPU-only checks of the voxel-grid field extraction (field_volume.py, njf_field_* in include/njf_hip.h): exported symbols,
host-side argument validation (nothing is launched: there is no GPU here), grid arithmetic and the PLY writer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_SYMBOLS = ("njf_field_points", "njf_field_select", "njf_field_forward")
E_NULL, E_SHAPE, E_ACTION_DIM, E_MODE, E_GMAP = -1, -2, -3, -6, -7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


def test_field_symbols_are_declared_exported_and_bound(lib):
    from neural_jacobian_field_amd import hip
    header = open(os.path.join(ROOT, "include", "njf_hip.h")).read()
    declared = set(re.findall(r"\b(njf_[a-z0-9_]+)\s*\(", header))
    for name in FIELD_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/njf_hip.h"
        assert name in hip.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert "typedef struct NjfFieldGrid" in header
    assert lib.njf_abi_version() == 20          # the change is additive
    assert int(re.search(r"#define NJF_FIELD_SELECT_BLOCK (\d+)", header).group(1)) == hip.FIELD_SELECT_BLOCK


def test_field_grid_struct_matches_the_header():
    from neural_jacobian_field_amd import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "njf_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct NjfFieldGrid \{(.*?)\} NjfFieldGrid;", header, flags=re.S).group(1)
    fields = re.findall(r"(float|int)\s+(\w+)\[3\];", body)
    assert fields == [("float", "origin"), ("float", "step"), ("int", "dims")]
    assert [f[0] for f in hip.FieldGrid._fields_] == [n for _, n in fields]
    assert C.sizeof(hip.FieldGrid) == 36


def _grid(dims=(4, 5, 6)):
    from neural_jacobian_field_amd import hip
    return hip.make_field_grid((0.0, 0.0, 1.0), (0.1, 0.1, 0.1), dims)


def test_field_points_and_select_validate_before_any_launch(lib):
    from neural_jacobian_field_amd import hip
    g, P = _grid(), 0x1000   # (a non-NULL stand-in pointer: validation failures return before it could be used)
    cams = hip.Cameras(P, P, None, None, None, None, None, 2, 0)
    pts, sel = lib.njf_field_points, lib.njf_field_select
    assert pts(None, 1, None, None, 8, P, None) == E_NULL                       # no grid
    assert pts(C.byref(g), 1, None, None, 8, None, None) == E_NULL              # no output
    assert pts(C.byref(g), 0, None, None, 8, P, None) == E_SHAPE                # batch < 1
    assert pts(C.byref(g), 1, None, None, -1, P, None) == E_SHAPE               # capacity < 0
    assert pts(C.byref(g), 1, None, None, 121, P, None) == E_SHAPE              # identity list longer than B*N = 120
    assert pts(C.byref(_grid((4, 0, 6))), 1, None, None, 8, P, None) == E_SHAPE  # dims < 1
    big = _grid((2048, 1024, 1024))                                             # N = 2^31: no int32 global index
    assert pts(C.byref(big), 1, None, None, 8, P, None) == E_SHAPE
    assert pts(C.byref(_grid((1024, 1024, 1024))), 2, None, None, 8, P, None) == E_SHAPE   # B*N = 2^31
    assert pts(C.byref(_grid((65536, 65536, 65536))), 1, None, None, 8, P, None) == E_SHAPE  # would overflow 64 bits naively
    assert pts(C.byref(g), 1, None, None, 0, P, None) == 0                      # nothing to do, nothing launched

    assert sel(None, None, 1, P, 0.5, None, None, 8, P, P, 8, P, None) == E_NULL
    assert sel(C.byref(g), None, 1, None, 0.5, None, None, 8, P, P, 8, P, None) == E_NULL      # no predicate at all
    assert sel(C.byref(g), None, 1, P, 0.5, None, None, 8, P, None, 8, P, None) == E_NULL      # no out_count
    assert sel(C.byref(g), None, 1, P, 0.5, None, None, 8, P, P, 8, None, None) == E_NULL      # no workspace
    assert sel(C.byref(g), None, 1, P, 0.5, None, None, 8, None, P, 8, P, None) == E_NULL      # capacity > 0 without out_indices
    assert sel(C.byref(g), None, 1, P, 0.5, None, None, 8, P, P, -1, P, None) == E_SHAPE       # output capacity < 0
    assert sel(C.byref(g), None, 1, P, 0.5, None, None, -1, P, P, 8, P, None) == E_SHAPE       # input capacity < 0
    assert sel(C.byref(g), C.byref(cams), 1, None, 0.0, None, None, 8, P, P, 8, P, None) == E_SHAPE   # cams.batch != batch
    no_k = hip.Cameras(P, None, None, None, None, None, None, 1, 0)
    assert sel(C.byref(g), C.byref(no_k), 1, None, 0.0, None, None, 8, P, P, 8, P, None) == E_NULL
    assert sel(C.byref(_grid((0, 1, 1))), None, 1, P, 0.5, None, None, 8, P, P, 8, P, None) == E_SHAPE


def test_field_forward_validates_before_any_launch(lib):
    from neural_jacobian_field_amd import hip
    g, P = _grid(), 0x1000
    cams = hip.Cameras(P, P, None, None, None, None, None, 1, 8)
    fmap = hip.FeatureMap(P, 8, 8, 768)
    fwd = lib.njf_field_forward
    w_c, w_j = P + 4 * hip.RESNET_W_FLOATS, P + 4 * (hip.RESNET_W_FLOATS + hip.COLOR_W_FLOATS)

    def call(grid=g, capacity=8, cam=cams, fm=fmap, goff_d=0, goff_j=384, mode=1, kind=1, w_d=P, b_d=P, wc=w_c, b_c=P, wj=w_j,
             b_j=P, density=P, color=P, jacobian=P, precision=2):
        return fwd(None if grid is None else C.byref(grid), None, None, capacity, None, None if cam is None else C.byref(cam),
                   None if fm is None else C.byref(fm), goff_d, goff_j, mode, kind, w_d, b_d, wc, b_c, wj, b_j, density, color,
                   jacobian, precision, None)

    assert call(grid=None) == E_NULL and call(cam=None) == E_NULL and call(fm=None) == E_NULL and call(w_d=None) == E_NULL
    assert call(capacity=-1) == E_SHAPE
    assert call(grid=_grid((3, 3, 0))) == E_SHAPE
    assert call(grid=_grid((2048, 1024, 1024))) == E_SHAPE
    assert call(capacity=121) == E_SHAPE                           # identity list longer than B*N
    assert call(mode=2) == E_MODE
    assert call(precision=4) == E_MODE and call(precision=0x13) == E_MODE   # unknown / f32 mixed with a split precision
    assert call(goff_d=2) == E_GMAP and call(goff_j=500) == E_GMAP          # misaligned / block past the map's stride
    assert call(kind=3) == E_MODE
    assert call(kind=1, cam=hip.Cameras(P, P, None, None, None, None, None, 1, 11)) == E_ACTION_DIM
    assert call(kind=1, jacobian=None) == E_NULL                   # a head without its output
    assert call(kind=1, wj=None) == E_NULL
    assert call(kind=0, color=P, wc=None) == E_NULL                # colour asked for without the colour head
    assert call(kind=1, wc=w_c + 4) == E_SHAPE                     # blobs not one allocation [density | colour | jacobian]
    assert call(kind=0, color=None, density=None) == E_NULL        # density-only pass without an output
    assert call(mode=0, density=None) == E_NULL
    assert call(capacity=0) == 0 and call(mode=0, capacity=0) == 0 and call(kind=0, color=None, capacity=0) == 0


def test_field_grid_index_and_coordinate_arithmetic():
    from neural_jacobian_field_amd.field_volume import FieldGrid
    grid = FieldGrid.from_bounds((-0.5, -0.25, 0.5), (0.5, 0.25, 2.0), (5, 3, 7))
    assert grid.dims == (5, 3, 7) and grid.num_nodes == 105
    assert grid.step == tuple(float(np.float32(s)) for s in (0.25, 0.25, 0.25))
    # linear index: z fastest, then y, then x -- and its inverse
    assert grid.linear_index(0, 0, 1) == 1 and grid.linear_index(0, 1, 0) == 7 and grid.linear_index(1, 0, 0) == 21
    n = np.arange(grid.num_nodes)
    ix, iy, iz = grid.unravel(n)
    assert np.array_equal(grid.linear_index(ix, iy, iz), n)
    assert np.array_equal(np.stack(grid.unravel(n + 3 * grid.num_nodes)), np.stack([ix, iy, iz]))   # global indices wrap per batch element
    xyz = grid.points()
    assert xyz.dtype == torch.float32 and tuple(xyz.shape) == (105, 3)
    assert torch.equal(xyz[0], torch.tensor([-0.5, -0.25, 0.5])) and torch.equal(xyz[-1], torch.tensor([0.5, 0.25, 2.0]))
    assert torch.equal(xyz[grid.linear_index(2, 1, 3)], torch.tensor([0.0, 0.0, 1.25]))
    picked = torch.tensor([104, 0, 105 + 50, 50])
    assert torch.equal(grid.points(picked), xyz[[104, 0, 50, 50]])
    # the coordinate is ONE rounding of i*step + origin (a fused multiply-add), not round(round(i*step) + origin)
    odd = FieldGrid((0.1, 0.1, 0.1), (1.0 / 3.0, 1e-3, 0.7), (50, 50, 50))
    got = odd.points().numpy().astype(np.float64)
    comps = odd.unravel(np.arange(odd.num_nodes))
    for c in range(3):
        exact = comps[c].astype(np.float64) * np.float64(np.float32(odd.step[c])) + np.float64(np.float32(odd.origin[c]))
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got[:, c] - exact) <= 0.5 * ulp * (1 + 1e-6))
    # one node on an axis sits at the lower bound; bad arguments are refused
    flat = FieldGrid.from_bounds((0, 0, 0), (1, 1, 1), (4, 1, 4))
    assert flat.step[1] == 0.0 and torch.all(flat.points()[:, 1] == 0)
    assert FieldGrid.from_bounds((0, 0, 0), (1, 1, 1), 3).dims == (3, 3, 3)
    for bad in ((0, 2, 2), (2, 2.5, 2)):
        with pytest.raises(ValueError):
            FieldGrid((0, 0, 0), (1, 1, 1), bad)
    with pytest.raises(ValueError):
        FieldGrid((0, 0, 0), (1, 1, 1), (2048, 1024, 1024))
    with pytest.raises(ValueError):
        FieldGrid.from_bounds((0, 0, 0), (1, 1, 1), (2, 0, 2))


def _read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    count = int([ln for ln in header if ln.startswith("element vertex")][0].split()[-1])
    kinds = {"float": "<f4", "uchar": "u1"}
    dtype = np.dtype([(ln.split()[2], kinds[ln.split()[1]]) for ln in header if ln.startswith("property")])
    assert len(raw) - end == count * dtype.itemsize
    return np.frombuffer(raw[end:], dtype=dtype, count=count)


def test_save_ply_round_trip(tmp_path):
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldPointCloud
    grid = FieldGrid.from_bounds((0, 0, 0), (1, 1, 1), 4)
    gen = torch.Generator().manual_seed(3)
    index = torch.tensor([1, 5, 9, 20, 63, 0, 0], dtype=torch.int32)      # 5 valid rows of 7 (a padded cloud)
    cloud = FieldPointCloud(grid=grid, index=index, xyz=grid.points(index), density=torch.rand(7, generator=gen) * 40,
                            color=torch.rand(7, 3, generator=gen), jacobian=torch.randn(7, 6, 3, generator=gen),
                            count=torch.tensor([5], dtype=torch.int32))
    assert cloud.valid() == 5 and torch.equal(cloud.batch_index, torch.zeros(7, dtype=torch.int32))
    path = tmp_path / "cloud.ply"
    assert cloud.save_ply(path) == 5
    v = _read_ply(path)
    assert v.dtype.names == ("x", "y", "z", "red", "green", "blue", "density") and len(v) == 5
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], -1), cloud.xyz[:5].numpy())
    assert np.array_equal(v["density"], cloud.density[:5].numpy())
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], -1), np.rint(cloud.color[:5].numpy() * 255).astype(np.uint8))
    # display colours of the Jacobians (the two point-cloud colour functions chained): [n, 3] in [0, 1], written on request
    cols = cloud.colors("model_toy_arm")
    assert tuple(cols.shape) == (5, 3) and float(cols.min()) >= 0.0 and float(cols.max()) <= 1.0
    from neural_jacobian_field_amd.inference import jacobian_color_map as cm
    table = torch.tensor(cm.JACOBIAN_COLORMAP["model_toy_arm"]).t()
    want = cm.visualize_joint_sensitivity_point_cloud(cm.compute_joint_sensitivity_point_cloud(cloud.jacobian[:5]), table)
    assert torch.equal(cols, want) and torch.equal(cloud.colors(table), want)
    cloud.save_ply(path, colors=cols)
    v = _read_ply(path)
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], -1), np.rint(cols.numpy() * 255).astype(np.uint8))
    with pytest.raises(ValueError):
        cloud.colors(torch.ones(3, 4))
    # an overfull capture-safe cloud (count > rows) writes the rows it has; an empty one writes a valid empty file
    cloud.count = torch.tensor([11], dtype=torch.int32)
    assert cloud.save_ply(path) == 7 and len(_read_ply(path)) == 7
    cloud.count = torch.tensor([0], dtype=torch.int32)
    assert cloud.save_ply(path) == 0 and len(_read_ply(path)) == 0


def test_extract_field_refuses_what_it_cannot_do_without_a_device():
    """flow_mlp has no Jacobian (the refusal of compute_jacobian_at), and bad options fail before any tensor is touched."""
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import FieldGrid, extract_field
    from neural_jacobian_field_amd.model import Model
    grid = FieldGrid.from_bounds((0, 0, 1), (1, 1, 2), 3)
    enc = PixelEncoding(features=torch.zeros(1, 512, 4, 4), extrinsics=torch.eye(4)[None], intrinsics=torch.eye(3)[None], action=None)
    flow = Model(model_cfg_from_dict({"action_dim": 4, "action_decoder": {"name": "flow_mlp"}}))
    with pytest.raises(NotImplementedError, match="no Jacobian"):
        extract_field(flow, enc, grid, 1.0)
    with pytest.raises(NotImplementedError, match="no Jacobian"):
        flow.decoder.compute_jacobian_at(None, enc)
    mlp = Model(model_cfg_from_dict({"action_dim": 4, "action_decoder": {"name": "jacobian_mlp"}}))
    with pytest.raises(ValueError):
        extract_field(mlp, enc, grid, float("nan"))
    with pytest.raises(ValueError):
        extract_field(mlp, enc, grid, 1.0, max_points=0)
    with pytest.raises(ValueError):
        extract_field(mlp, enc, grid, 1.0, view_direction=(0, 1))
    with pytest.raises(ValueError, match="GPU"):           # and there is no CPU path behind the checks
        extract_field(mlp, enc, grid, 1.0, in_frustum=False)
