"""GPU: the kernel every bf16 forward / adjoint entry launches is the one fmi_conv2d_bf16_plan names for the same descriptor, flags and
tile mode -- one launch per tile id per output stage, at the smallest shapes that reach each tile; fmi_debug_bf16_last_tile() is read
directly after the launch.  What the kernels compute is adjudicated elsewhere (test_gpu_bf16.py, test_gpu_vgg_bf16.py,
test_gpu_irse_infer_bf16.py, test_gpu_style_heads_bf16.py); the decisions themselves are pinned without a GPU in
test_host_conv_bf16_plan.py.  Operands are zeros: only the launch matters here.

The grouped case is G = 3, 64 -> 64, 3x3 stride 2 onto a 16 x 16 map (from 32 x 32): 256 output rows.  A 16 x 16 INPUT has 64 output rows,
which fmi_conv2d_grouped_fwd_bf16 gives to its weight-streaming kernel (at most FMI_STYLE_SKINNY_ROWS = 128 rows): no tile to record."""
import ctypes as C

import pytest
import torch

from face_mask_inpaint_amd import functional as FF

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
OUT_AL8 = 8  # FMI_PLAN_OUT_AL8: torch's allocations are aligned; no FMI_PLAN_MODES, so the query reads the tile mode the test sets
PLAIN, ACT, CHAN, GROUP, MASK = range(5)
ADJ_SHAPES = [(2, 8, 8, 64, 64), (1, 12, 20, 128, 64), (2, 16, 16, 256, 512), (2, 16, 16, 512, 256)]  # of tests/test_gpu_vgg_bf16.py
T64, T8P_512, T8P_256 = 64064, 1512128, 1256256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _z(dev, *shape, dtype=BF):
    return torch.zeros(shape, device=dev, dtype=dtype)


def _planned(d, pass_, stage, groups=1):
    out = (C.c_int * 14)()
    rc = FF._L().conv2d_bf16_plan(C.byref(d), pass_, stage, groups, OUT_AL8, C.cast(out, C.c_void_p))
    assert rc == 0 and out[0] == 0, (rc, list(out))
    return out[1]


def _launched():
    torch.cuda.synchronize()
    return FF._L().debug_bf16_last_tile()


def _other_tile_first(dev):
    """a 128 x 32 launch (1x40x40 32 -> 32, BK 32), so that the launch under test has to record its tile itself"""
    d, _, _ = FF.conv_desc(1, 40, 40, 32, 32, 3, 3, 1, 1)
    FF._L().conv2d_fwd_bf16(C.byref(d), FF._p(_z(dev, 1, 40, 40, 32)), FF._p(_z(dev, 32, 9, 32)), None, FF._p(_z(dev, 1, 40, 40, 32)), None, 0, FF._st())
    assert _launched() == 128032 == _planned(d, 0, PLAIN)


class _tile_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = FF._L().debug_bf16_tile(self.mode)

    def __exit__(self, *exc):
        FF._L().debug_bf16_tile(self.prev)
        return False


def _fwd(dev, shape, ks=3, stride=1, pad=1):
    n, h, w, c, k = shape
    d, oh, ow = FF.conv_desc(n, h, w, c, k, ks, ks, stride, pad)
    FF._L().conv2d_fwd_bf16(C.byref(d), FF._p(_z(dev, n, h, w, c)), FF._p(_z(dev, k, ks * ks, c)), None, FF._p(_z(dev, n, oh, ow, k)), None, 0, FF._st())
    return _launched(), _planned(d, 0, PLAIN)


def _adj(dev, shape, masked, ks=3, stride=1, pad=1):
    n, h, w, c, k = shape
    d, oh, ow = FF.conv_desc(n, h, w, c, k, ks, ks, stride, pad)
    dy, wck, dx = _z(dev, n, oh, ow, k), _z(dev, c, ks * ks, k), _z(dev, n, h, w, c)
    if masked:
        FF._L().conv2d_dgrad_relu_bf16(C.byref(d), FF._p(dy), FF._p(wck), FF._p(_z(dev, n, h, w, c)), FF._p(dx), FF._st())
    else:
        FF._L().conv2d_dgrad_bf16(C.byref(d), FF._p(dy), FF._p(wck), None, FF._p(dx), None, 0, FF._st())
    return _launched(), _planned(d, 1, MASK if masked else PLAIN)


# forward, plain stage: the six tiles of conv_bf16_kernel (128 x 32 at BK 32) -- (N, H, W, C -> K), tile mode, tile
FWD_CASES = [((1, 40, 40, 32, 32), 0, 128032), ((1, 192, 256, 64, 64), 0, 128064), ((2, 8, 8, 64, 64), 0, T64), ((1, 128, 128, 64, 128), 0, 64128),
             ((1, 128, 128, 64, 512), 0, 128128), ((1, 160, 160, 64, 512), 2, 256256)]
# adjoint, plain and masked stage: 64 x 64 at the four small shapes, the two eight-phase tiles under mode 8, and the four tiles that need rows
ADJ_CASES = ([(s, 0, T64) for s in ADJ_SHAPES] + [(ADJ_SHAPES[0], 8, T64), (ADJ_SHAPES[1], 8, T8P_512), (ADJ_SHAPES[2], 8, T8P_256), (ADJ_SHAPES[3], 8, T8P_256)]
             + [((1, 192, 256, 64, 64), 0, 128064), ((1, 128, 128, 128, 64), 2, 64128), ((1, 128, 128, 512, 64), 2, 128128), ((1, 160, 160, 512, 64), 2, 256256)])
_ids = lambda v: "N%d_%dx%d_%d-%d" % v if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.mark.parametrize("shape,mode,tile", FWD_CASES, ids=_ids)
def test_forward_runs_the_planned_tile(dev, shape, mode, tile):
    with _tile_mode(mode):
        assert _fwd(dev, shape) == (tile, tile)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape,mode,tile", ADJ_CASES, ids=_ids)
def test_adjoint_runs_the_planned_tile(dev, shape, mode, tile, masked):
    with _tile_mode(mode):
        assert _adj(dev, shape, masked) == (tile, tile)


def test_four_phase_adjoint_runs_the_planned_tile(dev):
    assert _adj(dev, (2, 9, 7, 64, 128), False, stride=2) == (T64, T64)


@pytest.mark.parametrize("k,tile", [(64, T8P_512), (256, T8P_256)])
def test_act_stage_runs_the_planned_tile(dev, k, tile):
    """the fused StyledConv stage exists on the eight-phase kernel only"""
    _other_tile_first(dev)
    d, _, _ = FF.conv_desc(2, 32, 32, 64, k, 3, 3, 1, 1)
    FF._L().conv2d_fwd_act_bf16(C.byref(d), FF._p(_z(dev, 2, 32, 32, 64)), FF._p(_z(dev, k, 9, 64)), None, None, None, None, 0.2, 1.0,
                                FF._p(_z(dev, 2, 32, 32, k)), FF._st())
    assert (_launched(), _planned(d, 0, ACT)) == (tile, tile)


@pytest.mark.parametrize("k,tile", [(64, 128064), (128, 128128)])
def test_chan_stage_records_and_runs_the_planned_tile(dev, k, tile):
    _other_tile_first(dev)
    d, _, _ = FF.conv_desc(2, 48, 48, 64, k, 3, 3, 1, 1)
    FF._L().conv2d_fwd_chan_bf16(C.byref(d), FF._p(_z(dev, 2, 48, 48, 64)), FF._p(_z(dev, k, 9, 64)), None, None, None, FF._p(_z(dev, 2, 48, 48, k)),
                                 None, 0, FF._st())
    assert (_launched(), _planned(d, 0, CHAN)) == (tile, tile)


@pytest.mark.parametrize("shared", [False, True], ids=["per_group", "shared"])
def test_grouped_stage_records_and_runs_the_planned_tile(dev, shared):
    _other_tile_first(dev)
    g, c, k = 3, 64, 64
    x = _z(dev, 1, 32, 32, c if shared else g * c)
    y = FF.conv2d_grouped_bf16(x, _z(dev, g, k, 9, c), _z(dev, g, k, dtype=torch.float32), 3, 2, 1, 0.01, shared)
    assert tuple(y.shape) == (1, 16, 16, g * k)
    if shared:  # one group of G K columns: the stacked packs are its weight
        d, _, _ = FF.conv_desc(1, 32, 32, c, g * k, 3, 3, 2, 1)
        want = _planned(d, 0, GROUP, 1)
    else:
        d, _, _ = FF.conv_desc(1, 32, 32, c, k, 3, 3, 2, 1, x_cs=g * c, y_cs=g * k)
        want = _planned(d, 0, GROUP, g)
    assert (_launched(), want) == (T64, T64)
