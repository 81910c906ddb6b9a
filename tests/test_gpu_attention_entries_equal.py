"""-m gpu: ey_area_attention and ey_flash_attention launch the same kernel (flash_attn_kernel<32>) and differ only in what a group is, so
handed the same groups they must return the same bytes: one area against the flash entry on the same views, and four areas whose runs
split rows against the flash entry on the same buffer viewed as one image per run (in NHWC a run is a contiguous pixel range)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from group_attn_util import data, lib  # noqa: E402

AREA_MFMA, FLASH_MFMA = 403, 500


def _qkv(B, H, W, heads, key):
    """q | k | v side by side in one f16 NHWC buffer (B, H, W, 3C)"""
    return torch.cat(data(B, H, W, heads, 32, key), 1).permute(0, 2, 3, 1).contiguous().to(device="cuda", dtype=torch.float16)


def _both(buf, heads, area):
    """-> output bytes of ey_area_attention on buf (B, H, W, 3C) and of ey_flash_attention on buf as B*area images of 1 x H*W/area"""
    from edge_yolo_amd.nn import _ops
    L = lib()
    B, H, W, C3 = buf.shape
    C = C3 // 3
    split = lambda b: [b.permute(0, 3, 1, 2)[:, j * C:(j + 1) * C] for j in range(3)]  # noqa: E731
    ya = _ops.area_attention(*split(buf), heads, area, 32 ** -0.5)
    assert L.lib().ey_attention_last_variant() == AREA_MFMA
    yf = _ops.flash_attention(*split(buf.view(B * area, 1, H * W // area, C3)), heads, 32 ** -0.5)
    assert L.lib().ey_attention_last_variant() == FLASH_MFMA + 32
    torch.cuda.synchronize()
    assert torch.isfinite(ya).all()
    return [y.permute(0, 2, 3, 1).contiguous().cpu().numpy().tobytes() for y in (ya, yf)]


@pytest.mark.parametrize("B,H,W,heads", [(2, 1, 17, 2), (1, 5, 13, 1), (2, 12, 20, 4)])  # 17, 65 and 240 tokens
def test_one_area_equals_flash(B, H, W, heads):
    a, f = _both(_qkv(B, H, W, heads, ("equal", H * W, heads)), heads, 1)
    assert a == f


def test_four_areas_equal_flash_on_runs():
    """2 x 6 x 10 map, 4 areas: runs of 15 tokens, one and a half rows each."""
    a, f = _both(_qkv(2, 6, 10, 2, ("equal", "runs")), 2, 4)
    assert a == f
