"""Column-interleaved planar activations [B][C/4][H][4 = x mod 4][W/4][4] behind the un-pooled fp32 F(4x4,3x3) layers
(conv_wino43.hip; forward.hip::plan_encoder decides per tensor) against the same tensors in NHWC (MP_DEBUG=no_xplanar).

The layout changes which addresses the producer's stores and the consumer's patch DMAs touch, not one multiply-add: the
outputs are EQUAL."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _net(oracle, cfg, seed):
    import multipoint_amd.models as M
    sd = oracle.make_weights(seed, cfg)
    net = M.MultiPoint(dict(cfg)); net.load_state_dict(sd); net.to('cuda'); net.eval()
    return net


# The tensors in question are conv3 -> conv4 at H/2 x W/2, conv5 -> conv6 at H/4 x W/4 and conv7 -> conv8 at H/8 x W/8; an item is 16 x 32
# pixels, or 32 x 16 where that covers the level with fewer items.  Every frame has reflected borders on all four sides.
#   (2, 96, 160)   48x80 (16x32 items, partial in both directions), 24x40 (32x16 items, partial), 12x20 (one partial 16x32 item)
#   (3, 64, 64)    32x32, 16x16, 8x8: single items, every patch pixel row / column of the border reflected
#   (5, 128, 96)   64x48 (32x16 items), 32x24 and 16x12 (16x32 items, partial)
#   (3, 72, 104)   36x52 (partial items); 18x26 and 9x13 are no multiples of the 4x4 tile: the any-frame kernel, NHWC (mixed forward)
#   (1, 240, 320)  120x160 (interior 16x32 items: the item-invariant offsets), 60x80 (32x16 items); 30x40 on the any-frame kernel
#   (3, 400, 320)  200x160 (interior 16x32 items), 100x80 (interior 32x16 items); 50x40 on the any-frame kernel
#   (1, 480, 640)  one pair at the shipped size: conv7 / conv8 run split-K, whose tensors stay NHWC
SHAPES = [(2, 96, 160), (3, 64, 64), (5, 128, 96), (3, 72, 104), (1, 240, 320), (3, 400, 320), (1, 480, 640)]


@pytest.mark.parametrize('upd', [{}, {'multispectral': True}, {'bn_first': True}])
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_xplanar_layout_is_bit_identical(oracle, monkeypatch, upd, B, H, W):
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    img = oracle.make_images(41 + W, B, H, W)
    flags = torch.tensor([[i % 2 == 0] for i in range(B)])
    a = _net(oracle, cfg, seed=9)({'image': img.cuda(), 'is_optical': flags})
    monkeypatch.setenv('MP_DEBUG', 'no_xplanar')
    b = _net(oracle, cfg, seed=9)({'image': img.cuda(), 'is_optical': flags})
    assert torch.equal(a['prob'], b['prob']) and torch.equal(a['desc'], b['desc'])
