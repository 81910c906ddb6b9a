"""Developer tool: one SHA-256 of the output bytes per case of a fixed list that covers every path of ey_area_attention and
ey_flash_attention, to prove a change leaves the bits alone: run it on the build before and the build after and diff the listings.
Inputs come from integer arithmetic only -- ((i * 2654435761 + seed) mod 4096 - 2048) / 1024, exact in f16 -- so they are the same on
any torch build.  Each line: case, ey_attention_last_variant, digest.  The area-1 MFMA cases and the flash head_dim 32 cases share their
inputs, so their digests agree with each other too.
usage: attn_bits.py"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import edge_yolo_amd  # noqa: E402,F401
from edge_yolo_amd import _lib as L  # noqa: E402
from edge_yolo_amd.nn import _ops as ops  # noqa: E402

# tokens -> (B, H, W)
MAPS = {17: (2, 1, 17), 60: (2, 6, 10), 65: (1, 5, 13), 240: (2, 12, 20), 401: (1, 1, 401), 1600: (2, 40, 40)}
F16, F32 = torch.float16, torch.float32
# (entry, tokens, area, heads, head_dim, dtype, channel offset of q in its buffer, areaattn_mfma)
CASES = [("area", n, 1, h, 32, F16, 0, 1) for n, h in ((17, 2), (65, 1), (240, 4), (401, 1))]
CASES += [("area", 60, 4, 2, 32, F16, 0, 1), ("area", 1600, 4, 2, 32, F16, 0, 1)]                 # runs of 15 (split rows) and 400
CASES += [("area", 60, 4, 2, 32, F32, 0, 1), ("area", 240, 1, 4, 32, F32, 0, 1)]                  # fp32 VALU
CASES += [("area", 60, 4, 2, 32, F16, 0, 0), ("area", 65, 1, 1, 32, F16, 0, 0), ("area", 60, 4, 2, 16, F16, 0, 1),
          ("area", 65, 1, 2, 64, F16, 0, 1)]                                                    # f16 VALU: knob at 0, head_dim 16 / 64
CASES += [("flash", n, 1, h, hd, F16, 0, 1) for hd in (16, 32, 64) for n, h in ((17, 2), (65, 1), (240, 4), (401, 1))]
CASES += [("flash", 65, 1, 2, 32, F32, 0, 1), ("flash", 240, 1, 1, 16, F32, 0, 1)]                # fp32 VALU
CASES += [("flash", 65, 1, 2, 32, F16, 4, 1), ("flash", 17, 1, 2, 24, F16, 0, 1)]                 # f16 VALU: unaligned q, head_dim 24


def fill(shape, seed):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    return (((i * 2654435761 + seed) % 4096 - 2048).double() / 1024).view(shape)


for entry, n, area, heads, hd, dtype, off, knob in CASES:
    B, H, W = MAPS[n]
    C = heads * hd
    buf = fill((B, H, W, off + 3 * C), 1000 * n + 10 * heads + hd).to(dtype).cuda().permute(0, 3, 1, 2)
    q, k, v = (buf[:, off + j * C:off + (j + 1) * C] for j in range(3))
    L.check(L.lib().ey_tune_set(b"areaattn_mfma", knob), "tune")
    y = ops.area_attention(q, k, v, heads, area, hd ** -0.5) if entry == "area" else ops.flash_attention(q, k, v, heads, hd ** -0.5)
    variant = L.lib().ey_attention_last_variant()
    L.check(L.lib().ey_tune_set(b"areaattn_mfma", 1), "tune")
    torch.cuda.synchronize()
    digest = hashlib.sha256(y.permute(0, 2, 3, 1).contiguous().cpu().numpy().tobytes()).hexdigest()
    name = f"{entry} {'f16' if dtype == F16 else 'f32'} N{n} area{area} h{heads} hd{hd}" + (f" qoff{off}" if off else "") + ("" if knob else " knob0")
    print(f"{name:44s} {variant:3d} {digest}", flush=True)
