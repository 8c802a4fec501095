"""Which precision codes and which action dimensions the decoder entries take: hip.precision_code / Model(...) on the Python side
against valid_precision / check_jacobian of the C side, reached through njf_render_forward in the manner of
tests/row_entries_cases.py.  Every call here carries a fault that is judged AFTER the thing under test, so nothing launches and no
pointer is followed: the structs hold the address ``P``, samples = 1, and
  * for the codes, a feature map whose stride is no multiple of 4: a refused code returns NJF_E_MODE, an accepted one goes on
    to the stride and returns NJF_E_GMAP;
  * for the action dimension, a good map and a colour blob that does NOT follow the density blob: a refused A returns
    NJF_E_ACTION_DIM, an accepted one goes on to the contiguity of the blobs and returns NJF_E_SHAPE."""
import ctypes as C
import itertools

import pytest

P = 0x1000
E_SHAPE, E_ACTION_DIM, E_MODE, E_GMAP = -2, -3, -6, -7


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    hip.load_library()
    return hip


def render_code(hip, precision: int, stride: int = 1027, action_dim: int = 8, kind: int = 1) -> int:
    """The return code of njf_render_forward for ``precision`` on a [1, 4, 4, stride] map with an A-channel head of ``kind``."""
    cams = hip.Cameras(P, P, P, P, P, P, P, 1, action_dim)
    fmap = hip.FeatureMap(P, 4, 4, stride)
    out = hip.RenderOutputs()
    # (w_color = P does not follow w_density = P: check_contiguous refuses whatever passed every check before it)
    return hip.load_library().njf_render_forward(P, P, 3, C.byref(cams), C.byref(fmap), 0, 384, kind, P, P, P, P, P, P, P, 1,
                                                 C.byref(out), precision, None)


def mixed(hip, d: str, j: str) -> int:
    return hip.PRECISIONS[d] | ((hip.PRECISIONS[j] + 1) << 4)      # include/njf_hip.h: NJF_PRECISION_MIXED(d, j)


def test_the_c_side_accepts_exactly_six_codes(hip):
    accepted = sorted(p for p in [-1, *range(256), 256] if render_code(hip, p) != E_MODE)
    assert accepted == sorted([0, 1, 2, 3, mixed(hip, "f16x2", "f16f6"), mixed(hip, "f16f6", "f16x2")]), accepted
    assert all(render_code(hip, p) == E_GMAP for p in accepted)     # ... and those went on to the next check
    assert [hip.PRECISIONS[k] for k in ("f32", "f16x2", "f16f6", "f16")] == [0, 1, 2, 3]
    # the order inside a mixed code: density in the low nibble, head above it
    assert mixed(hip, "f16x2", "f16f6") == 0x31 and mixed(hip, "f16f6", "f16x2") == 0x22


def test_precision_code_raises_exactly_where_the_c_side_refuses(hip):
    names = sorted(hip.PRECISIONS)
    seen = {}
    for d, j in itertools.product(names, names):
        try:
            code = hip.precision_code(d, j)
        except ValueError:
            code = None
        want = mixed(hip, d, j) if d != j else hip.PRECISIONS[d]    # the code this pair WOULD have
        refused = render_code(hip, want) == E_MODE
        assert (code is None) == refused, (d, j, code, want)
        if code is not None:
            assert code == want, (d, j, code, want)
            seen[(d, j)] = code
    assert len(set(seen.values())) == len(seen) == 6, seen           # one code per accepted pair, six pairs
    assert hip.precision_code("f16f6", None) == hip.precision_code("f16f6", "f16f6") == 2
    for bad in (("f8", None), ("f16x2", "f8")):
        with pytest.raises(ValueError, match="unknown precision"):
            hip.precision_code(*bad)


@pytest.mark.parametrize("kind,name,limit", [(1, "jacobian_mlp", 10), (2, "jacobian_transformer", 8)])
def test_action_dimension_limits_of_the_two_heads(hip, kind, name, limit):
    """ResnetFC head: A <= NJF_MAX_ACTION_DIM = 10 (30 of the 32 output rows); transformer head: 8 key slots.  Model(...) and the ABI
    draw the line at the same place, the ABI before any launch."""
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model
    stride = 384 + (384 if kind == 1 else 64)      # NJF_ZDIM channels of the density block, then the head's block
    for a in range(0, 13):
        for precision in (0, 1, 2, mixed(hip, "f16x2", "f16f6"), mixed(hip, "f16f6", "f16x2")):
            code = render_code(hip, precision, stride=stride, action_dim=a, kind=kind)
            assert code == (E_SHAPE if 1 <= a <= limit else E_ACTION_DIM), (name, a, precision, code)
    cfg = lambda a: model_cfg_from_dict({"action_dim": a, "encoder": {"name": "precomputed"},
                                         "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                                         "action_decoder": {"name": name}})
    assert Model(cfg(limit)).decoder.action_dim == limit
    with pytest.raises(ValueError, match="action_dim"):
        Model(cfg(limit + 1))


def test_transformer_head_refuses_nine_channels_and_the_resnetfc_head_takes_ten(hip):
    """The two statements of the limits spelled out: jacobian_transformer with A = 9 is refused by Model(...) and by the ABI
    (NJF_E_ACTION_DIM); jacobian_mlp with A = 10 passes the same checks."""
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model
    cfg = lambda name, a: model_cfg_from_dict({"action_dim": a, "encoder": {"name": "precomputed"},
                                               "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                                               "action_decoder": {"name": name}})
    with pytest.raises(ValueError):
        Model(cfg("jacobian_transformer", 9))
    assert render_code(hip, 2, stride=448, action_dim=9, kind=2) == E_ACTION_DIM
    assert Model(cfg("jacobian_mlp", 10)).decoder.jacobian_head.lin_out.weight.shape == (30, 128)
    assert render_code(hip, 2, stride=768, action_dim=10, kind=1) == E_SHAPE
