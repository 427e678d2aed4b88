"""CPU: ``aggregate.pixel_strides`` — which (N, C, H, W) tensors count as pixel-major (channels-last) and
with which (node stride, pixel stride) — and the ``set_channels_last`` switch.  Strides only: no GPU."""
import pytest
import torch

from mrp_gnn_amd import aggregate
from mrp_gnn_amd.aggregate import node_stride, pixel_strides

N, C, H, W = 3, 6, 4, 5
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _cl(n, c, h, w, dtype=torch.float32):
    return torch.zeros(n, c, h, w, dtype=dtype).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_channels_last(dtype):
    t = _cl(N, C, H, W, dtype)
    assert t.stride() == (H * W * C, 1, W * C, C)
    assert node_stride(t) is None
    assert pixel_strides(t) == (H * W * C, C)


def test_both_halves_of_a_channels_last_cat_buffer():
    buf = _cl(N, 2 * C, H, W)
    for half in (buf[:, :C], buf[:, C:]):
        assert node_stride(half) is None
        assert pixel_strides(half) == (H * W * 2 * C, 2 * C)


def test_channel_slice_of_a_wider_buffer():
    buf = _cl(N, C + 2, H, W)
    assert pixel_strides(buf[:, 1:C + 1]) == (H * W * (C + 2), C + 2)


def test_node_slices_and_single_node():
    t = _cl(N, C, H, W)
    assert pixel_strides(t[::2]) == (2 * H * W * C, C)     # node stride > H W ps
    one = _cl(1, C, H, W)
    assert pixel_strides(one) == (H * W * C, C)            # N == 1: any s[0]
    assert pixel_strides(t[1:2]) == (H * W * C, C)
    assert pixel_strides(one.as_strided((1, C, H, W), (7, 1, W * C, C))) == (H * W * C, C)


def test_node_major_wins_every_ambiguous_case():
    assert pixel_strides(_cl(N, 1, H, W)) is None          # C == 1
    assert node_stride(_cl(N, 1, H, W)) is not None
    assert pixel_strides(_cl(N, C, 1, 1)) is None          # H * W == 1
    assert node_stride(_cl(N, C, 1, 1)) is not None
    nchw = torch.zeros(N, C, H, W)
    assert node_stride(nchw) == C * H * W and pixel_strides(nchw) is None
    assert pixel_strides(torch.zeros(N, 2 * C, H, W)[:, C:]) is None   # half of an NCHW cat buffer


def test_single_row_or_column_planes():
    assert pixel_strides(_cl(N, C, H, 1)) == (H * C, C)
    assert pixel_strides(_cl(N, C, 1, W)) == (W * C, C)


def test_neither_layout_is_none():
    t = torch.zeros(N, H, W, C)
    assert pixel_strides(t.permute(0, 3, 2, 1)) is None    # (N, C, W, H) view: pixels in the other order
    assert node_stride(t.permute(0, 3, 2, 1)) is None
    wide = torch.zeros(N, H, W + 1, C).permute(0, 3, 1, 2)[:, :, :, :W]   # row pitch != W * ps
    assert pixel_strides(wide) is None
    assert pixel_strides(_cl(N, 2 * C, H, W)[:, ::2]) is None             # channel stride 2
    assert pixel_strides(_cl(N, C, H, W).double()) is None                # not a feature dtype
    assert pixel_strides(torch.zeros(N, C, H)) is None
    assert pixel_strides(_cl(N, C, H, W).as_strided((N, C, H, W), (0, 1, W * C, C))) is None  # overlapping nodes


def test_set_channels_last_returns_the_previous_value():
    assert aggregate.set_channels_last("convert") == "native"   # the default
    try:
        assert aggregate.set_channels_last("convert") == "convert"
        with pytest.raises(ValueError):
            aggregate.set_channels_last("nhwc")
    finally:
        assert aggregate.set_channels_last("native") == "convert"
    assert aggregate.set_channels_last("native") == "native"
