"""-m gpu: every dispatch branch of the MFMA conv operator (conv2d_typed, csrc/conv_igemm.inc.h) and the depthwise / DSConv kernels
against an fp64 reference (tests/fp64_ref.py), in both dtypes.

* Exact matrix: integer inputs in [-2, 2], weights in multiples of 1/4, biases / addz / residual in multiples of 1/4, power-of-two
  out_scale, act none / ReLU.  Every partial sum is exact in fp32 in any summation order, so the kernel output must be BIT-IDENTICAL
  to the fp64 result.  Each case forces its branch with the existing tunables and asserts the launched kernel label.
* Single-tap probes: one non-zero pixel per image (corner, tile seam, last row / column) -- the output is the shifted weight pattern.
* Schedules: the persistent / XCD-ordered kernels repeat ragged cases with grid_div = 7 and xcd_map = 0 (same bits).
* Bounded (f16, SiLU, general data): the per-element fp64 bound and the mean-ulp gate of fp64_ref.report, the fast epilogues included.
* The benchmarked step: every conv-family label of a batch-32 and a batch-1 forward at 640x640 is covered here (COVERED), and every
  distinct conv2d call of both forwards is replayed at its exact shape / views with exact data.  Block programs are not excused:
  every block_ label of the step is in test_gpu_block_exact.BLOCK_COVERED and every recorded chain is replayed AS A CHAIN."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_ref as R  # noqa: E402
from gpu_util import _traced, tuned  # noqa: E402

NONE, SILU, RELU = R.ACT_NONE, R.ACT_SILU, R.ACT_RELU
DT = [torch.float16, torch.float32]
_HUGE = 1 << 40
# forcing sets (existing tunables only)
PW = dict()                                      # lean pointwise: the default below 110 000 output pixels
PWN = dict(pw_m=0)                               # N-split pointwise
PWR = dict(pw_m=0, pwn=0, pwr_m=0)               # register-stationary pointwise at any size
SMALL = dict(pw_m=0, pwn=0)                      # small-M 1x1
OFF3 = dict(c3r=0, c3s=0, c3p=0, tile_mink=_HUGE)  # every f16-only 3x3 kernel off
TILE = dict(c3r=0, c3s=0, c3p=0, tile_s2_minm=0, tile_minwg=0)
HALO = dict(OFF3)
WS1 = dict(pw_m=0, pwn=0, pwr_m=_HUGE, small_m=0)
WS3 = dict(OFF3, halo_min_c=_HUGE)
IGEMM = dict(OFF3, halo_min_c=_HUGE, ws_k3_minnt=8)


def C(name, cin, cout, k, s, B, H, W, tune, l16, l32, **kw):
    d = dict(name=name, cin=list(cin), cout=cout, k=k, s=s, B=B, H=H, W=W, tune=tune, l16=l16, l32=l32, up=None, addz=False, res=False,
             out_scale=1.0, view=False, out_slice=False, act=NONE, ngroup=1, sched=False, probe=False)
    d.update(kw)
    return d


def _pw(nt):
    return f"conv_pw_kernel<{{t}},{nt}>"


# label templates: {t} = f16 / f32.  l32 = the kernel the f32 parity mode takes for the same call.
CASES = [
    # ---- conv_pw: each NT, one / two sources, upsampled source, epilogue operands
    C("pw_nt1", [24], 12, 1, 1, 3, 7, 9, PW, _pw(1), _pw(1), view=True, out_slice=True),
    C("pw_nt2", [40], 40, 1, 1, 3, 11, 13, PW, _pw(2), _pw(2), act=RELU),
    C("pw_nt4", [48], 64, 1, 1, 5, 100, 100, PW, _pw(4), "conv_ws_kernel<{t},4,1,1>"),
    C("pw_nt5", [72], 80, 1, 1, 5, 100, 99, PW, _pw(5), "conv_ws_kernel<{t},5,1,1>"),
    C("pw_nt8", [32], 128, 1, 1, 5, 100, 100, PW, _pw(8), "conv_ws_kernel<{t},8,1,1>"),
    C("pw_cin80", [80], 40, 1, 1, 3, 9, 11, PW, _pw(2), _pw(2), view=True),
    C("pw_2src_up", [32, 16], 68, 1, 1, 3, 10, 14, PW, _pw(1), _pw(1), up=[0, 1]),
    C("pw_addz_res_scale", [64], 64, 1, 1, 2, 10, 12, PW, _pw(2), _pw(2), addz=True, res=True, out_scale=0.5, out_slice=True),
    # ---- conv_pwn: KS x NTW (pwn_ntw), two sources with an upsampled one
    C("pwn_ks4", [128], 128, 1, 1, 3, 19, 23, dict(PWN, pwn_ntw=1), "conv_pwn_kernel<{t},4,1>", None),
    C("pwn_ks6_ntw2", [128, 64], 256, 1, 1, 3, 20, 22, dict(PWN, pwn_ntw=2), "conv_pwn_kernel<{t},6,2>", None, up=[0, 1]),
    C("pwn_ks4_ntw2", [128], 256, 1, 1, 3, 19, 23, dict(PWN, pwn_ntw=2), "conv_pwn_kernel<{t},4,2>", "conv_small_kernel<{t},2,4>"),
    C("pwn_ks6_ntw1", [192], 128, 1, 1, 2, 17, 31, dict(PWN, pwn_ntw=1), "conv_pwn_kernel<{t},6,1>", "conv_small_kernel<{t},2,4>"),
    C("pwn_ks8_ntw2", [256], 256, 1, 1, 3, 13, 29, dict(PWN, pwn_ntw=2), "conv_pwn_kernel<{t},8,2>", "conv_small_kernel<{t},2,4>"),
    C("pwn_ks8", [256], 128, 1, 1, 2, 25, 27, dict(PWN, pwn_ntw=1), "conv_pwn_kernel<{t},8,1>", None, view=True),
    C("pwn_ks12_ntw2", [384], 256, 1, 1, 3, 21, 17, dict(PWN, pwn_ntw=2), "conv_pwn_kernel<{t},12,2>", None),
    C("pwn_ks12_ntw1", [384], 256, 1, 1, 1, 40, 40, dict(PWN, pwn_ntw=1), "conv_pwn_kernel<{t},12,1>", None),
    C("pwn_ks16_ntw2", [512], 256, 1, 1, 5, 15, 15, dict(PWN, pwn_ntw=2), "conv_pwn_kernel<{t},16,2>", None, out_slice=True),
    C("pwn_ks16_ntw1", [512], 128, 1, 1, 3, 20, 20, dict(PWN, pwn_ntw=1), "conv_pwn_kernel<{t},16,1>", None),
    # ---- conv_pwr: KS 1-4, TWO / GEO
    C("pwr_ks1", [32], 16, 1, 1, 3, 13, 17, PWR, "conv_pwr_kernel<{t},1,1>", None, sched=True),
    C("pwr_ks2", [40], 32, 1, 1, 3, 9, 11, PWR, "conv_pwr_kernel<{t},2,2>", None, view=True),
    C("pwr_ks3", [96], 64, 1, 1, 1, 1, 1, PWR, "conv_pwr_kernel<{t},4,3>", None),
    C("pwr_ks4", [128], 64, 1, 1, 2, 15, 13, PWR, "conv_pwr_kernel<{t},4,4>", None, res=True, out_slice=True),
    C("pwr_nt5", [48], 80, 1, 1, 3, 7, 5, PWR, "conv_pwr_kernel<{t},5,2>", None),
    C("pwr_nt8_two", [32, 48], 128, 1, 1, 3, 9, 13, PWR, "conv_pwr_kernel<{t},8,3>", None),
    C("pwr_two_geo", [32, 32], 64, 1, 1, 3, 10, 14, PWR, "conv_pwr_kernel<{t},4,2>", None, up=[0, 1], sched=True),
    C("pwr_nt2_ks1", [32], 32, 1, 1, 5, 9, 7, PWR, "conv_pwr_kernel<{t},2,1>", None),
    # regression: Cout 40 is not a whole 16*NT tile -- conv_pwr stores whole channel groups and wrote 24 channels past each pixel
    # (the neighbour's first channels, past the end of the view at the last pixel); the dispatcher now leaves such shapes to other kernels
    C("pwr_cout_tail", [32, 32], 40, 1, 1, 3, 10, 14, PWR, "conv_small_kernel<{t},4,8>", "conv_small_kernel<{t},2,4>", up=[0, 1]),
    C("pwr_geo_addz", [64], 64, 1, 1, 2, 12, 10, PWR, "conv_pwr_kernel<{t},4,2>", None, addz=True, out_scale=0.25, res=True),
    # ---- conv_small
    C("small_m1", [96], 80, 1, 1, 1, 1, 1, SMALL, "conv_small_kernel<{t},5,8>", "conv_small_kernel<{t},1,4>"),
    C("small_nt4", [48], 64, 1, 1, 3, 5, 7, SMALL, "conv_small_kernel<{t},4,8>", "conv_small_kernel<{t},2,4>", act=RELU),
    C("small_nt1", [40], 12, 1, 1, 3, 6, 5, SMALL, "conv_small_kernel<{t},1,8>", "conv_small_kernel<{t},1,4>", out_slice=True),
    C("small_2src", [64, 32], 128, 1, 1, 2, 6, 8, SMALL, "conv_small_kernel<{t},4,8>", "conv_small_kernel<{t},2,4>", up=[1, 0], res=True),
    # ---- conv3r (Cin 16): stride 1 (c3r = 2) and 2
    C("c3r_s1", [16], 16, 3, 1, 3, 13, 37, dict(c3r=2), "conv3r_kernel<1,1>", None, sched=True),
    C("c3r_s2", [16], 32, 3, 2, 3, 27, 33, dict(c3r=2), "conv3r_kernel<2,2>", None, sched=True, view=True),
    C("c3r_s2_12", [16], 12, 3, 2, 1, 9, 9, dict(c3r=2), "conv3r_kernel<1,2>", None, out_slice=True),
    # ---- conv3s: S1 / S2 x MT2 / MT4 (c3s_cfg = MT * 10 + ring depth 3)
    C("c3s_s1_mt4", [64], 64, 3, 1, 3, 21, 19, dict(c3s=2, c3s_cfg=43), "conv3s_kernel<4,4,1>", None, sched=True),
    C("c3s_s1_mt2", [128], 64, 3, 1, 2, 13, 11, dict(c3s=2, c3s_cfg=23), "conv3s_kernel<4,2,1>", None, view=True),
    C("c3s_s2_mt4", [128], 128, 3, 2, 3, 23, 25, dict(c3s=2, c3s_cfg=43), "conv3s_kernel<4,4,2>", None, sched=True),
    C("c3s_s2_mt2", [64], 40, 3, 2, 5, 15, 18, dict(c3s=2, c3s_cfg=23), "conv3s_kernel<4,2,2>", None, res=True, out_slice=True),
    C("c3s_s1_nt2", [256], 64, 3, 1, 2, 7, 9, dict(c3s=2), "conv3s_kernel<2,2,1>", None),
    C("c3s_s2_nt1", [64], 12, 3, 2, 1, 1, 1, dict(c3s=2), "conv3s_kernel<1,2,2>", None),
    # ---- conv3p (Cin 64, stride 1), generic epilogue (act none; the fast one: bounded SiLU cases)
    C("c3p_64", [64], 64, 3, 1, 3, 21, 24, dict(c3p=2), "conv3p_kernel<4>", None),
    C("c3p_128", [64], 128, 3, 1, 2, 9, 40, dict(c3p=2), "conv3p_kernel<4>", None, view=True),
    C("c3p_40_res", [64], 40, 3, 1, 3, 11, 13, dict(c3p=2), "conv3p_kernel<4>", None, res=True, out_slice=True),
    # ---- conv3_tile: S1 / S2 x tile_wlds x tile_flat
    C("tile_s1_nt4", [24], 40, 3, 1, 3, 13, 37, dict(TILE, tile_wlds=1, tile_flat=1), "conv3_tile_kernel<{t},4,1>", None, sched=True),
    C("tile_s1_cin80", [80], 64, 3, 1, 2, 11, 19, dict(TILE, tile_wlds=1), "conv3_tile_kernel<{t},4,1>", "conv_ws_kernel<{t},1,1,3>", view=True),
    C("tile_s1_nt1", [72], 12, 3, 1, 2, 17, 9, dict(TILE, tile_wlds=0, tile_flat=0), "conv3_tile_kernel<{t},1,1>", None, view=True),
    C("tile_s1_nt2", [32], 32, 3, 1, 3, 10, 41, dict(TILE, tile_wlds=2, tile_flat=1), "conv3_tile_kernel<{t},2,1>", None, res=True),
    C("tile_s1_flat0", [48], 64, 3, 1, 1, 19, 45, dict(TILE, tile_wlds=1, tile_flat=0), "conv3_tile_kernel<{t},4,1>", None, out_slice=True),
    C("tile_s2_nt4", [64], 64, 3, 2, 3, 25, 33, dict(TILE, tile_wlds=1), "conv3_tile_kernel<{t},4,2>", None, sched=True),
    C("tile_s2_nt1", [96], 16, 3, 2, 2, 18, 31, dict(TILE, tile_wlds=0), "conv3_tile_kernel<{t},1,2>", None),
    C("tile_s2_wlds2", [128], 128, 3, 2, 1, 16, 20, dict(TILE, tile_wlds=2), "conv3_tile_kernel<{t},4,2>", None),
    # ---- conv3_halo (Cin 48..64)
    C("halo_s1", [48], 80, 3, 1, 3, 17, 35, HALO, "conv3_halo_kernel<{t},5,1>", None),
    C("halo_s2", [64], 40, 3, 2, 2, 19, 21, HALO, "conv3_halo_kernel<{t},4,2>", None, res=True),
    # ---- conv_ws: MT1 / MT2, k 1 / 3
    C("ws_k1_mt1", [72], 80, 1, 1, 3, 9, 13, WS1, "conv_ws_kernel<{t},5,1,1>", None, sched=True),
    C("ws_k1_mt2", [40], 68, 1, 1, 3, 11, 9, dict(WS1, mt2_min_m=0), "conv_ws_kernel<{t},5,2,1>", None, addz=False, out_slice=True),
    C("ws_k1_2src", [32, 32], 64, 1, 1, 2, 10, 14, WS1, "conv_ws_kernel<{t},4,1,1>", None, up=[1, 0], addz=True, out_scale=2.0),
    C("ws_k3_mt1", [24], 40, 3, 1, 3, 13, 15, WS3, "conv_ws_kernel<{t},4,1,3>", None, sched=True),
    C("ws_k3_mt2_s2", [96], 128, 3, 2, 3, 17, 19, dict(WS3, mt2_min_m=0), "conv_ws_kernel<{t},2,2,3>", "conv_ws_kernel<{t},1,2,3>", res=True),
    C("ws_k3_nt2", [128], 128, 3, 2, 1, 80, 80, WS3, "conv_ws_kernel<{t},2,1,3>", "conv_ws_kernel<{t},1,1,3>"),
    # ---- K-chunked fallback
    C("igemm_mt1", [256], 128, 3, 1, 3, 9, 11, IGEMM, "conv_igemm_kernel<{t},8,1>", None),
    C("igemm_mt2", [256], 128, 3, 2, 2, 363, 363, IGEMM, "conv_igemm_kernel<{t},8,2>", None),
    # ---- grouped form (wavelet sub-band convs: ngroup 4, weight set min(g, 1))
    C("group_tile", [32], 16, 3, 1, 3, 10, 12, dict(), "conv3_tile_kernel<{t},1,1>", None, ngroup=4, act=RELU),
    C("group_ws", [32], 16, 3, 1, 2, 9, 7, WS3, "conv_ws_kernel<{t},1,1,3>", None, ngroup=4),
    # ---- single-tap probes: stride 1 and 2 per 3x3 family
    C("probe_c3r_s1", [16], 16, 3, 1, 3, 17, 40, dict(c3r=2), "conv3r_kernel<1,1>", None, probe=True),
    C("probe_c3r_s2", [16], 32, 3, 2, 3, 33, 35, dict(c3r=2), "conv3r_kernel<2,2>", None, probe=True),
    C("probe_c3s_s1", [64], 64, 3, 1, 3, 17, 40, dict(c3s=2, c3s_cfg=43), "conv3s_kernel<4,4,1>", None, probe=True),
    C("probe_c3s_s2", [128], 64, 3, 2, 3, 33, 35, dict(c3s=2, c3s_cfg=23), "conv3s_kernel<4,2,2>", None, probe=True),
    C("probe_c3p_s1", [64], 64, 3, 1, 3, 17, 40, dict(c3p=2), "conv3p_kernel<4>", None, probe=True),
    C("probe_tile_s1", [32], 64, 3, 1, 3, 17, 40, dict(TILE), "conv3_tile_kernel<{t},4,1>", None, probe=True),
    C("probe_tile_s2", [64], 64, 3, 2, 3, 33, 35, dict(TILE), "conv3_tile_kernel<{t},4,2>", None, probe=True),
    C("probe_halo_s1", [64], 80, 3, 1, 3, 17, 40, HALO, "conv3_halo_kernel<{t},5,1>", None, probe=True),
    C("probe_halo_s2", [48], 80, 3, 2, 3, 33, 35, HALO, "conv3_halo_kernel<{t},5,2>", None, probe=True),
    C("probe_ws_s1", [24], 40, 3, 1, 3, 17, 40, WS3, "conv_ws_kernel<{t},4,1,3>", None, probe=True),
    C("probe_ws_s2", [40], 40, 3, 2, 3, 33, 35, WS3, "conv_ws_kernel<{t},4,1,3>", None, probe=True),
    C("probe_igemm_s1", [256], 128, 3, 1, 3, 17, 40, IGEMM, "conv_igemm_kernel<{t},8,1>", None, probe=True),
    C("probe_igemm_s2", [256], 128, 3, 2, 3, 33, 35, IGEMM, "conv_igemm_kernel<{t},8,1>", None, probe=True),
]
_BY_NAME = {c["name"]: c for c in CASES}
assert len(_BY_NAME) == len(CASES)

# Depthwise / DSConv: (name, kind, C, Cout, k, B, H, W, tune, l16, l32, sched)
DW_CASES = [
    ("dw3", "dw", 80, 80, 3, 3, 13, 17, dict(), "dwconv_kernel<3>", "dwconv_kernel<3>", True),
    ("dw5", "dw", 32, 32, 5, 2, 9, 31, dict(), "dwconv_kernel<5>", "dwconv_kernel<5>", False),
    ("ds_strip3", "ds", 48, 40, 3, 3, 11, 13, dict(), "dsconv_strip_kernel<3>", "dsconv_kernel<3>", True),
    ("ds_strip7", "ds", 64, 64, 7, 2, 10, 9, dict(), "dsconv_strip_kernel<7>", "dsconv_kernel<7>", False),
    ("ds_strip5_c32", "ds", 32, 32, 5, 3, 7, 11, dict(tz_kmask=0), "dsconv_strip_kernel<5>", "dsconv_kernel<5>", False),
    ("ds_tile3", "ds", 32, 32, 3, 1, 40, 40, dict(ds_strip=0, tz_kmask=0), "dsconv_kernel<3>", "dsconv_kernel<3>", False),  # batch-1 step shape
    ("ds_tz3", "ds", 32, 24, 3, 3, 13, 15, dict(tz_minpx=0), "dsconv_tz_kernel<3>", "dsconv_kernel<3>", True),
    ("ds_tz5", "ds", 16, 16, 5, 2, 9, 20, dict(tz_minpx=0), "dsconv_tz_kernel<5>", "dsconv_kernel<5>", False),
    ("ds_tz7", "ds", 32, 32, 7, 3, 17, 19, dict(), "dsconv_tz_kernel<7>", "dsconv_kernel<7>", True),
]

SCHED = [dict(grid_div=7), dict(xcd_map=0)]


def _tn(dtype):
    return "f16" if dtype == torch.float16 else "f32"


def _expected(case, dtype):
    lab = case["l16"] if dtype == torch.float16 else (case["l32"] or F32_LABELS.get(case["name"]))
    return lab.format(t=_tn(dtype)) if lab else None


# The f32 parity mode has none of the f16-only kernels (pwn, pwr, c3r, c3s, c3p, tile): the same calls take these.
F32_LABELS = {
    "pwn_ks4": "conv_small_kernel<{t},2,4>", "pwn_ks6_ntw2": "conv_small_kernel<{t},2,4>", "pwn_ks8": "conv_small_kernel<{t},2,4>", "pwn_ks12_ntw2": "conv_small_kernel<{t},2,4>",
    "pwn_ks12_ntw1": "conv_small_kernel<{t},2,4>", "pwn_ks16_ntw2": "conv_small_kernel<{t},2,4>", "pwn_ks16_ntw1": "conv_small_kernel<{t},2,4>",
    "pwr_ks1": "conv_small_kernel<{t},1,4>", "pwr_ks2": "conv_small_kernel<{t},2,4>", "pwr_ks3": "conv_small_kernel<{t},2,4>",
    "pwr_ks4": "conv_small_kernel<{t},2,4>", "pwr_nt5": "conv_small_kernel<{t},1,4>", "pwr_nt8_two": "conv_small_kernel<{t},2,4>",
    "pwr_two_geo": "conv_small_kernel<{t},2,4>", "pwr_nt2_ks1": "conv_small_kernel<{t},2,4>", "pwr_geo_addz": "conv_small_kernel<{t},2,4>",
    "c3r_s1": "conv_ws_kernel<{t},1,1,3>", "c3r_s2": "conv_ws_kernel<{t},2,1,3>", "c3r_s2_12": "conv_ws_kernel<{t},1,1,3>",
    "c3s_s1_mt4": "conv3_halo_kernel<{t},1,1>", "c3s_s1_mt2": "conv_ws_kernel<{t},1,1,3>", "c3s_s2_mt4": "conv_ws_kernel<{t},1,1,3>",
    "c3s_s2_mt2": "conv_ws_kernel<{t},1,1,3>", "c3s_s1_nt2": "conv_ws_kernel<{t},1,1,3>", "c3s_s2_nt1": "conv_ws_kernel<{t},1,1,3>",
    "c3p_64": "conv3_halo_kernel<{t},1,1>", "c3p_128": "conv3_halo_kernel<{t},1,1>", "c3p_40_res": "conv3_halo_kernel<{t},1,1>",
    "tile_s1_nt4": "conv_ws_kernel<{t},4,1,3>", "tile_s1_nt1": "conv_ws_kernel<{t},1,1,3>", "tile_s1_nt2": "conv_ws_kernel<{t},2,1,3>",
    "tile_s1_flat0": "conv3_halo_kernel<{t},2,1>", "tile_s2_nt4": "conv_ws_kernel<{t},1,1,3>", "tile_s2_nt1": "conv_ws_kernel<{t},1,1,3>",
    "tile_s2_wlds2": "conv_ws_kernel<{t},1,1,3>", "halo_s1": "conv3_halo_kernel<{t},1,1>", "halo_s2": "conv_ws_kernel<{t},1,1,3>",
    "ws_k1_mt1": "conv_ws_kernel<{t},5,1,1>", "ws_k1_mt2": "conv_ws_kernel<{t},5,2,1>", "ws_k1_2src": "conv_ws_kernel<{t},4,1,1>",
    "ws_k3_mt1": "conv_ws_kernel<{t},4,1,3>",
    "igemm_mt1": "conv_igemm_kernel<{t},8,1>", "igemm_mt2": "conv_igemm_kernel<{t},8,2>",
    "group_tile": "conv_ws_kernel<{t},1,1,3>", "group_ws": "conv_ws_kernel<{t},1,1,3>",
    "probe_c3r_s1": "conv_ws_kernel<{t},1,1,3>", "probe_c3r_s2": "conv_ws_kernel<{t},2,1,3>", "probe_c3s_s1": "conv3_halo_kernel<{t},1,1>",
    "probe_c3s_s2": "conv_ws_kernel<{t},1,1,3>", "probe_c3p_s1": "conv3_halo_kernel<{t},1,1>", "probe_tile_s1": "conv_ws_kernel<{t},2,1,3>",
    "probe_tile_s2": "conv_ws_kernel<{t},1,1,3>", "probe_halo_s1": "conv3_halo_kernel<{t},1,1>", "probe_halo_s2": "conv3_halo_kernel<{t},1,2>",
    "probe_ws_s1": "conv_ws_kernel<{t},4,1,3>", "probe_ws_s2": "conv_ws_kernel<{t},2,1,3>", "probe_igemm_s1": "conv_igemm_kernel<{t},8,1>",
    "probe_igemm_s2": "conv_igemm_kernel<{t},8,1>",
}

# Conv-family kernels of the step that other test files check: each against its multi-launch form and, at every parametrized shape
# (the benchmark's included), against fp64 with the fused-chain bound of fp64_ref.check_chain
FUSED_COVERED = {
    "stem_kernel": "test_gpu_ops.py::test_stem_mfma_agrees_with_f32_kernel",
    "stem_pair_kernel": "test_gpu_stem_pair.py",
    "pw3_kernel": "test_gpu_pw3.py",
    "conv_pwc_kernel<f16,4>": "test_gpu_pwc.py", "conv_pwc_kernel<f16,8>": "test_gpu_pwc.py",
    "conv_pw2_kernel": "test_gpu_ops.py::test_pointwise_chain_kernel_agrees_with_two_f32_convs",
    "dsb_pair_kernel<3,5>": "test_gpu_dsb.py", "dsb_pair_kernel<3,7>": "test_gpu_dsb.py",
}


def covered_labels():
    """Every f16 kernel label this module (and FUSED_COVERED) checks against fp64 -- the step runs in f16, and some labels
    (dsconv_kernel<k>, dwconv_kernel<k>) carry no dtype, so the f32 runs do not count."""
    out = set(FUSED_COVERED)
    for c in CASES:
        out.add(_expected(c, torch.float16))
    for d in DW_CASES:
        out.add(d[9])
    return out


# ------------------------------------------------------------------------------------------------------------------------ helpers
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _holder():
    from edge_yolo_amd.nn import modules as M
    return M.Conv(8, 8, 1)  # only its packed-weight cache is used (a fresh one per call: packed weights are cached on the module)


def _nhwc(B, c, H, W, dtype, vals=None, pad=0):
    """NHWC device tensor; pad > 0: a channel slice [8, 8 + c) of a (c + pad)-channel buffer whose other channels hold NaN (a kernel
    that reads outside its view, even into a zero-padded weight column, turns the output into NaN)."""
    from edge_yolo_amd import _lib as L
    if pad:
        buf = L.empty_nhwc(B, c + pad, H, W, dtype, "cuda")
        buf.copy_(torch.full((B, c + pad, H, W), float("nan")))
        t = buf[:, 8:8 + c]
    else:
        t = L.empty_nhwc(B, c, H, W, dtype, "cuda")
    if vals is not None:
        t.copy_(vals)
    return t


def _probe_input(B, c, H, W, gen):
    """zeros except one pixel per image: corner, a tile seam, the last row / column (cycled over the batch)."""
    x = torch.zeros(B, c, H, W, dtype=torch.float64)
    spots = [(0, 0), (min(8, H - 1), min(16, W - 1)), (H - 1, W - 1), (min(7, H - 1), W - 1), (H - 1, min(31, W - 1))]
    for b in range(B):
        y, xx = spots[b % len(spots)]
        v = torch.randint(1, 3, (c,), generator=gen).double() * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1)
        x[b, :, y, xx] = v
    return x


def _data(case, dtype, act, gen, general=False):
    """inputs, weights, bias, addz, res for one case: exact dyadic data (default) or general data (bounded checks)."""
    B, H, W, k, s = case["B"], case["H"], case["W"], case["k"], case["s"]
    up = case["up"] or [0] * len(case["cin"])
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    cin, cout, ng = sum(case["cin"]), case["cout"], case["ngroup"]
    nsets = 2 if ng > 1 else 1
    K = cin * k * k
    xs = []
    for c, u in zip(case["cin"], up):
        shp = (B, c * ng, H >> u, W >> u)
        if general:
            xs.append(torch.randn(shp, generator=gen).half().double())
        elif case["probe"]:
            xs.append(_probe_input(*shp, gen))
        else:
            xs.append(R.ex_input(shp, gen))
    ws, bs = [], []
    for _ in range(nsets):
        if general:
            ws.append((torch.randn((cout, cin, k, k), generator=gen) * (2.0 / K) ** 0.5).half().double())
            bs.append(torch.randn(cout, generator=gen).float() * 0.5)
        else:
            ws.append(R.ex_sparse_weight((cout, cin, k, k), gen, R.safe_density(K, 100.0)))
            bs.append(R.ex_bias(cout, gen))
    z = None
    if case["addz"]:
        z = torch.randn((B, cout, Ho // 2, Wo // 2), generator=gen).half().double() if general else R.ex_input((B, cout, Ho // 2, Wo // 2), gen) / 4
    r = None
    if case["res"]:
        r = torch.randn((B, cout, Ho, Wo), generator=gen).half().double() if general else R.ex_input((B, cout, Ho, Wo), gen) / 4
    return xs, ws, bs, z, r, (Ho, Wo)


def run_case(case, dtype, act=None, extra_tune=None, general=False):
    """Launch one case through nn._ops.conv2d; returns (list of (kernel output, fp64 reference y, A, Y)), launched labels, raw variant."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    act = case["act"] if act is None else act
    gen = _gen(case["name"], str(dtype), act, general)
    xs, ws, bs, z, r, (Ho, Wo) = _data(case, dtype, act, gen, general)
    B, k, s, cout, ng = case["B"], case["k"], case["s"], case["cout"], case["ngroup"]
    up = case["up"] or [0] * len(xs)
    pad = 16 if case["view"] else 0
    srcs = [_nhwc(B, x.shape[1], x.shape[2], x.shape[3], dtype, x, pad) for x in xs]
    zd = _nhwc(B, cout, Ho // 2, Wo // 2, dtype, z) if z is not None else None
    rd = _nhwc(B, cout, Ho, Wo, dtype, r) if r is not None else None
    wq = [w.to(dtype).double() for w in ws]  # what the packed weights hold (exact data: unchanged)
    kw = {}
    if ng > 1:
        c = case["cin"][0]
        out_buf = _nhwc(B, ng * cout, Ho, Wo, dtype, torch.full((B, ng * cout, Ho, Wo), 5.0))
        out = out_buf[:, :cout]
        kw = dict(ngroup=ng, src_gstride=c, y_gstride=cout, w_sets=2)
        fn = lambda: [(w.float(), b) for w, b in zip(ws, bs)]  # noqa: E731
        srcs = [srcs[0][:, :c]]
    else:
        fn = lambda: (ws[0].float(), bs[0])  # noqa: E731
        out_buf, out = None, None
        if case["out_slice"]:
            out_buf = _nhwc(B, cout + 24, Ho, Wo, dtype, torch.full((B, cout + 24, Ho, Wo), 5.0))
            out = out_buf[:, 16:16 + cout]
    t = dict(case["tune"])
    t.update(extra_tune or {})
    with tuned(**t):
        got, labels = _traced(lambda: _ops.conv2d(_holder(), srcs, fn, k, s, k // 2, act, out=out, res=rd, up=list(up), addz=zd,
                                                  out_scale=case["out_scale"], **kw))
        lv = L.lib().ey_conv_last_variant()
    res = []
    if ng > 1:
        full = xs[0].cuda()
        c = case["cin"][0]
        for g in range(ng):
            y, A, Y = R.conv_ref([full[:, g * c:(g + 1) * c]], wq[min(g, 1)], bs[min(g, 1)], k, s, k // 2, act)
            res.append((out_buf[:, g * cout:(g + 1) * cout], y, A, Y))
    else:
        y, A, Y = R.conv_ref([x.cuda() for x in xs], wq[0], bs[0], k, s, k // 2, act, up=list(up), addz=z.cuda() if z is not None else None,
                             out_scale=case["out_scale"], res=r.cuda() if r is not None else None)
        res.append((got, y, A, Y))
        if out_buf is not None:  # neighbouring channels of the output buffer untouched
            keep = torch.cat([out_buf[:, :16], out_buf[:, 16 + cout:]], 1)
            assert bool((keep == 5.0).all()), f"{case['name']}: conv wrote outside its output channel slice"
    return res, labels, lv, wq


def _check_label(name, labels, want):
    assert len(labels) == 1, f"{name}: expected one launch, got {labels}"
    if want is not None:
        assert labels[0] == want, f"{name}: launched {labels[0]}, expected {want}"


# ------------------------------------------------------------------------------------------------------------------------ §2 exact
@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_conv_exact(name, dtype):
    case = _BY_NAME[name]
    res, labels, _, _ = run_case(case, dtype)
    for i, (got, y, _, _) in enumerate(res):
        R.assert_exact(f"{name} {_tn(dtype)} g{i}", labels[0], got, y)
    _check_label(name, labels, _expected(case, dtype))


@pytest.mark.parametrize("sched", SCHED, ids=["grid_div7", "xcd_map0"])
@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["sched"]])
def test_conv_exact_schedules(name, sched):
    """persistent grids (grid_div) and XCD-contiguous work orders (xcd_map) on ragged tile counts: the same exact bits."""
    case = _BY_NAME[name]
    res, labels, _, _ = run_case(case, torch.float16, extra_tune=sched)
    _check_label(name, labels, _expected(case, torch.float16))
    for got, y, _, _ in res:
        R.assert_exact(f"{name} {sched}", labels[0], got, y)


def _dw_run(kind, c, cout, k, B, H, W, dtype, gen, general=False, act=NONE):
    """depthwise (kind 'dw': ey_dwconv) or fused DSConv ('ds': dw -> f16 intermediate -> pw 1x1) on exact or general data."""
    from edge_yolo_amd.nn import _ops
    if general:
        x = torch.randn((B, c, H, W), generator=gen).half().double()
        wd = (torch.randn((c, 1, k, k), generator=gen) / k).to(dtype).double()
        wp = (torch.randn((cout, c, 1, 1), generator=gen) * (2.0 / c) ** 0.5).to(dtype).double()
        bd, bp = torch.randn(c, generator=gen).float() * 0.2, torch.randn(cout, generator=gen).float() * 0.5
    else:
        x = R.ex_input((B, c, H, W), gen)
        wd, wp = R.ex_weight((c, 1, k, k), gen), R.ex_weight((cout, c, 1, 1), gen)
        bd, bp = R.ex_bias(c, gen), R.ex_bias(cout, gen)
    xd = _nhwc(B, c, H, W, dtype, x)
    dense = torch.zeros((c, c, k, k), dtype=torch.float64)
    dense[torch.arange(c), torch.arange(c)] = wd[:, 0]
    if kind == "dw":
        got, labels = _traced(lambda: _ops.dwconv(_holder(), xd, lambda: (wd.float(), bd), k, act))
        y, A, Y = R.conv_ref([x.cuda()], dense, bd, k, 1, k // 2, act)
        return got, labels, (y, A, Y, k * k), None
    # DSConv: the depthwise stage (bias, no activation) is kept as f16 before the pointwise conv (fp32 in f32 mode)
    got, labels = _traced(lambda: _ops.dsconv(_holder(), xd, lambda: (wd.float(), bd.float()), lambda: (wp.float(), bp), k, act))
    m, mA, mY = R.conv_ref([x.cuda()], dense, bd, k, 1, k // 2, NONE)
    mid = m.to(dtype).double()
    y, A, Y = R.conv_ref([mid], wp, bp, 1, 1, 0, act)
    return got, labels, (y, A, Y, c), (m, mA, mY, k * k + 1, mid, wp)


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("case", DW_CASES, ids=[d[0] for d in DW_CASES])
def test_dw_dsconv_exact(case, dtype):
    name, kind, c, cout, k, B, H, W, tune, l16, l32, _ = case
    with tuned(**tune):
        got, labels, (y, _, _, _), _ = _dw_run(kind, c, cout, k, B, H, W, dtype, _gen(name, str(dtype)))
    R.assert_exact(f"{name} {_tn(dtype)}", labels[0], got, y)
    _check_label(name, labels, l16 if dtype == torch.float16 else l32)


@pytest.mark.parametrize("sched", SCHED, ids=["grid_div7", "xcd_map0"])
@pytest.mark.parametrize("case", [d for d in DW_CASES if d[-1]], ids=[d[0] for d in DW_CASES if d[-1]])
def test_dw_dsconv_exact_schedules(case, sched):
    name, kind, c, cout, k, B, H, W, tune, l16, _, _ = case
    with tuned(**dict(tune, **sched)):
        got, labels, (y, _, _, _), _ = _dw_run(kind, c, cout, k, B, H, W, torch.float16, _gen(name, "sched"))
    _check_label(name, labels, l16)
    R.assert_exact(f"{name} {sched}", labels[0], got, y)


# ------------------------------------------------------------------------------------------------------------------------ §3 bounded
BOUNDED = [c["name"] for c in CASES if not c["probe"]]


@pytest.mark.parametrize("name", BOUNDED)
def test_conv_f16_silu_within_fp64_bound(name):
    """general data (f16 inputs / weights, fp32 bias), SiLU: per-element fp64 bound + mean-ulp gate; c3p without epilogue operands
    takes its deferred fast epilogue here (asserted)."""
    case = _BY_NAME[name]
    res, labels, lv, _ = run_case(case, torch.float16, act=SILU, general=True)
    _check_label(name, labels, _expected(case, torch.float16))
    if name == "c3p_64" or name == "c3p_128":
        assert lv % 10 == 1, f"{name}: conv3p fast epilogue not taken (variant {lv})"
    K = R.nterms(sum(case["cin"]), case["k"], case["addz"])
    for i, (got, y, A, Y) in enumerate(res):
        R.report(f"{name} silu g{i}", labels[0], got, y, R.bound(y, A, Y, K, case["out_scale"]))


@pytest.mark.parametrize("case", DW_CASES, ids=[d[0] for d in DW_CASES])
def test_dw_dsconv_f16_silu_within_fp64_bound(case):
    """DSConv: two-stage bound -- the f16 intermediate is rounded where the kernel rounds it; its error propagates through |w_pw|."""
    name, kind, c, cout, k, B, H, W, tune, l16, _, _ = case
    with tuned(**tune):
        got, labels, (y, A, Y, K2), mid = _dw_run(kind, c, cout, k, B, H, W, torch.float16, _gen(name, "silu"), general=True, act=SILU)
    _check_label(name, labels, l16)
    if mid is None:
        R.report(f"{name} silu", labels[0], got, y, R.bound(y, A, Y, K2 + 1))
        return
    m, mA, mY, K1, midr, wp = mid
    b1 = R.bound(m, mA, mY, K1)  # depthwise stage: fp32 accumulation + the f16 rounding of the intermediate
    inherited = R.propagate(R.mid_error(b1, midr), wp, 1, 1, 0)
    R.report(f"{name} silu", labels[0], got, y, R.bound(y, A, Y, K2 + 1) + inherited)


# ------------------------------------------------------------------------------------------------------------------------ §4 the step
_FAMILY = ("conv", "stem", "pw3", "dsb_pair", "dsconv", "dwconv")
_STEP = {}
_STEP_CHAINS = {}  # batch -> the chains BlockCache.run recorded during the forward (tag, input views, their conv2d calls, output pointers)


def _step_forward(batch):
    """One eager f16 forward of the benchmark model at 640x640 under the tracer, every nn._ops.conv2d call recorded.

    Eager, not bench.py's pipelined runner: the runner replays captured hipGraphs, and the tracer brackets the Python wrapper of each
    launch with HIP events, which a graph replay never passes through -- there are no per-launch labels to collect there.  The
    kernels are the same: every dispatch rule reads only the call's shape, views and tunables, which the runner's stages share with
    this forward (same model, same batch, same 640x640 input).  Layers the forward runs as a block program (nn/_block.py) go through
    block_tile_kernel in both; their conv2d calls are recorded twice over: one by one (replayed through ey_conv2d at the same shape)
    and grouped by the BlockCache.run that recorded them (_STEP_CHAINS: replayed as a chain through block_tile_kernel)."""
    if batch in _STEP:
        return _STEP[batch]
    import bench
    from edge_yolo_amd.nn import _block, _ops
    from edge_yolo_amd import _lib as L
    m, _ = bench.build_model("yolo11n-test.yaml", torch.float16, "cuda")
    calls, chains = [], []
    orig = _ops.conv2d
    orig_run = _block.BlockCache.run

    def ptr(t):
        t = L.as_nhwc(t)
        return (t.data_ptr(), t.untyped_storage().data_ptr())

    def run_rec(cache, fn, ins, outs=None):
        n0 = len(calls)
        got = orig_run(cache, fn, ins, outs)
        if got is not None and len(calls) > n0:  # recorded in this call: the chain's conv2d calls, in order
            def vw(t):
                t = L.as_nhwc(t)
                return ((tuple(t.shape), L.cstride(t), (t.data_ptr() - t.untyped_storage().data_ptr()) // t.element_size() % L.cstride(t)), t.untyped_storage().data_ptr())
            chains.append(dict(tag=cache.tag, tiled=cache.tiled, ins=[vw(t) for t in ins], calls=calls[n0:], outs={L.as_nhwc(t).data_ptr() for t in got}))
        return got

    def rec(mod, srcs, folded_fn, k, s, p, act, out=None, res=None, tag="", up=None, addz=None, out_scale=1.0, ngroup=1, src_gstride=0, y_gstride=0,
            group_C=None, w_sets=1, _build_only=False):
        n0 = len(_ops.TRACE.records) if _ops.TRACE is not None else 0
        r = orig(mod, srcs, folded_fn, k, s, p, act, out=out, res=res, tag=tag, up=up, addz=addz, out_scale=out_scale, ngroup=ngroup,
                 src_gstride=src_gstride, y_gstride=y_gstride, group_C=group_C, w_sets=w_sets, _build_only=_build_only)
        if not _build_only and r is not None:
            lab = _ops.TRACE.records[-1][0] if _ops.TRACE is not None and len(_ops.TRACE.records) > n0 else None

            def view(t):
                if t is None:
                    return None
                t = L.as_nhwc(t)
                base = t.untyped_storage().data_ptr()
                return (tuple(t.shape), L.cstride(t), (t.data_ptr() - base) // t.element_size() % L.cstride(t))
            ss, up2 = srcs, up
            if len(ss) == 1 and isinstance(ss[0], _ops.VirtualCat):
                vc = ss[0]
                if k == 1 and len(vc.parts) <= 2 and up is None:
                    ss, up2 = [t for t, _ in vc.parts], [u for _, u in vc.parts]
                else:  # the conv read a freshly materialized dense tensor
                    ss, up2 = [None], None
            sv = [view(t) if t is not None else (tuple(srcs[0].shape), srcs[0].shape[1], 0) for t in ss]
            w = folded_fn()
            cout = (w[0][0] if w_sets > 1 else w[0]).shape[0]
            calls.append(dict(srcs=sv, up=list(up2 or [0] * len(ss)), k=k, s=s, p=p, act=act, out=view(r if out is None else out),
                              res=view(res), addz=view(addz), out_scale=float(out_scale), ngroup=ngroup, src_gstride=src_gstride, y_gstride=y_gstride,
                              group_C=group_C, w_sets=w_sets, cout=cout, label=lab,
                              ptrs=dict(srcs=[ptr(t) if t is not None else None for t in ss], out=ptr(r if out is None else out),
                                        res=ptr(res) if res is not None else None)))
        return r

    x = torch.rand((batch, 3, 640, 640), generator=torch.Generator().manual_seed(batch)).half().cuda()
    _ops.conv2d = rec
    _block.BlockCache.run = run_rec
    try:
        with torch.no_grad():
            _, labels = _traced(lambda: m(x))
    finally:
        _ops.conv2d = orig
        _block.BlockCache.run = orig_run
    del m, x
    torch.cuda.empty_cache()
    _STEP[batch] = (labels, calls)
    _STEP_CHAINS[batch] = chains
    return _STEP[batch]


@pytest.mark.parametrize("batch", [32, 1])
def test_step_conv_kernels_are_covered(batch):
    labels, _ = _step_forward(batch)
    fam = sorted({lab for lab in labels if lab.startswith(_FAMILY)})
    print(f"[step] batch {batch} at 640x640: {len(fam)} conv-family kernels: {fam}")
    assert fam, "no conv-family launch traced"
    missing = sorted(set(fam) - covered_labels())
    assert not missing, f"batch {batch}: conv-family kernels of the step that no exact / bounded case covers: {missing}"


def _replay_key(c):
    return repr({k: v for k, v in c.items() if k not in ("label", "ptrs")})


def _replay_one(c, gen):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    dtype = torch.float16
    k, s, p, cout, ng = c["k"], c["s"], c["p"], c["cout"], c["ngroup"]
    assert c["group_C"] is None

    def make(v, vals=None, fill=float("nan")):  # channels outside the view: NaN (inputs) or a sentinel (the output buffer)
        (B, ch, H, W), cs, off = v
        buf = L.empty_nhwc(B, cs, H, W, dtype, "cuda")
        buf.copy_(torch.full((B, cs, H, W), fill))
        t = buf[:, off:off + ch]
        if vals is not None:
            t.copy_(vals)
        return buf, t

    xs, srcs, bufs = [], [], []
    for v, u in zip(c["srcs"], c["up"]):
        (B, ch, H, W), cs, off = v
        if ng > 1:  # the groups are channel-offset slices of one buffer: fill all of them
            buf, t = make(v)
            full = R.ex_input((B, cs, H, W), gen)
            buf.copy_(full)
            xs.append(full)
        else:
            x = R.ex_input((B, ch, H, W), gen)
            buf, t = make(v, x)
            xs.append(x)
        srcs.append(t)
        bufs.append(buf)
    cin = sum(v[0][1] for v in c["srcs"])
    K = cin * k * k
    # with addz the bilinear weights (1/16 .. 9/16) and the 1/2 scale leave multiples of 1/32: |y| must stay below 64 to be exact in f16
    ws = [R.ex_sparse_weight((cout, cin, k, k), gen, R.safe_density(K, 25.0 if c["addz"] is not None else 100.0)) for _ in range(c["w_sets"])]
    bs = [R.ex_bias(cout, gen) for _ in range(c["w_sets"])]
    fn = (lambda: [(w.float(), b) for w, b in zip(ws, bs)]) if c["w_sets"] > 1 else (lambda: (ws[0].float(), bs[0]))
    z = r = zd = rd = None
    if c["addz"] is not None:
        z = R.ex_input(c["addz"][0], gen)
        _, zd = make(c["addz"], z)
    if c["res"] is not None:
        r = R.ex_input(c["res"][0], gen) / 4
        _, rd = make(c["res"], r)
    obuf, out = make(c["out"], fill=5.0)
    if ng > 1:
        out = obuf[:, c["out"][2]:c["out"][2] + cout]
    scale = 0.5 if c["out_scale"] != 1.0 else 1.0  # a power of two; != 1 wherever the step's call had a learned scale (same dispatch)
    got, labels = _traced(lambda: _ops.conv2d(_holder(), srcs, fn, k, s, p, NONE, out=out, res=rd, up=list(c["up"]), addz=zd, out_scale=scale,
                                              ngroup=ng, src_gstride=c["src_gstride"], y_gstride=c["y_gstride"], w_sets=c["w_sets"]))
    outs = []
    if ng > 1:
        gs = c["src_gstride"]
        ch = c["srcs"][0][0][1]
        off = c["srcs"][0][2]
        for g in range(ng):
            xg = xs[0][:, off + g * gs: off + g * gs + ch].cuda()
            y, _, _ = R.conv_ref([xg], ws[min(g, c["w_sets"] - 1)], bs[min(g, c["w_sets"] - 1)], k, s, p, NONE)
            o0 = c["out"][2] + g * c["y_gstride"]
            outs.append((obuf[:, o0:o0 + cout], y))
    else:
        y, _, _ = R.conv_ref([x.cuda() for x in xs], ws[0], bs[0], k, s, p, NONE, up=list(c["up"]), addz=z.cuda() if z is not None else None,
                             out_scale=scale, res=r.cuda() if r is not None else None)
        outs.append((got, y))
    mask = torch.ones(obuf.shape[1], dtype=torch.bool)
    o0 = c["out"][2]
    for g in range(ng):
        mask[o0 + g * c["y_gstride"]:o0 + g * c["y_gstride"] + cout] = False
    if bool(mask.any()):  # channels of the output buffer outside the conv's output views stay untouched
        assert bool((obuf[:, mask.cuda()] == 5.0).all()), "conv wrote outside its output channel slice"
    return labels, outs


@pytest.mark.parametrize("batch", [32, 1])
def test_step_conv_calls_replay_exact(batch):
    """every distinct conv2d call of the step, at its exact shape, views, groups and epilogue operands, with exact data: bit-identical
    to fp64, through the same kernel instantiation the step launched.  (Calls recorded into a block program run inside
    block_tile_kernel in the step and have no label of their own; here they go through ey_conv2d at the same shape, and
    test_step_block_chains_replay_exact runs them again as the chain they were recorded into.)"""
    _, calls = _step_forward(batch)
    seen = {}
    for c in calls:
        seen.setdefault(_replay_key(c), c)
    assert seen, "no conv2d call recorded"
    print(f"[replay] batch {batch}: {len(calls)} conv2d calls, {len(seen)} distinct")
    cov = covered_labels()
    for i, (key, c) in enumerate(seen.items()):
        labels, outs = _replay_one(c, _gen("replay", batch, i))
        assert len(labels) == 1
        if c["label"] is not None:
            assert labels[0] == c["label"], f"replay of {key} launched {labels[0]}, the step launched {c['label']}"
        assert labels[0] in cov, f"{labels[0]} ({key}) is not covered by the exact matrix"
        for j, (got, y) in enumerate(outs):
            R.assert_exact(f"replay b{batch} #{i} g{j} {c['srcs'][0][0]}->{c['cout']} k{c['k']}s{c['s']}", labels[0], got, y)
        torch.cuda.empty_cache()


@pytest.mark.parametrize("batch", [32, 1])
def test_step_block_chains_replay_exact(batch):
    """every block_ label of the step is held to fp64 by test_gpu_block_exact.py (BLOCK_COVERED), and every chain the forward recorded
    is replayed AS A CHAIN through block_tile_kernel: the step's shapes, channel strides and offsets, the same dataflow (LDS-resident
    intermediates, the in-place write over the input slice, the read-back), exact data (ReLU / none in place of SiLU): bit for bit."""
    import test_gpu_block_exact as BE
    labels, _ = _step_forward(batch)
    blk = sorted({lab for lab in labels if lab.startswith("block_")})
    chains = _STEP_CHAINS[batch]
    print(f"[step] batch {batch}: block programs {blk}; recorded chains {[(c['tag'], len(c['calls'])) for c in chains]}")
    assert blk, "no block program traced: the default pointwise chain of C2PSA_LinearAttention did not run"
    missing = sorted(set(blk) - set(BE.BLOCK_COVERED))
    assert not missing, f"batch {batch}: block programs of the step that test_gpu_block_exact.py does not cover: {missing}"
    assert {f"block_tile_kernel<{c['tag']}>" if c["tiled"] else f"block_kernel<{c['tag']}>" for c in chains} == set(blk), "a traced block program was not recorded"
    for i, ch in enumerate(chains):
        assert ch["tiled"], ch["tag"]
        ntis = BE.replay_step_chain(ch, i)
        print(f"[step] batch {batch}: chain {ch['tag']} replayed exact, tile_nti {ntis}")
