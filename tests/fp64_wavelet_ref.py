"""fp64 reference of the fused half-resolution wavelet branch (nn._ops.wavelet_z, csrc/wavelet.hip) and its per-element bound,
plus the data recipes the CPU and the GPU tests of that kernel share.

The kernel keeps four f16 tensors (three in LDS): the sub-bands, (use_ds) the depthwise 3x3 output, P and Z.  The reference runs the
same four stages in float64 and rounds to f16 at exactly those points; each stage's bound is fp64_ref.bound (fp32 accumulation of K
terms in any order, the fp32 SiLU, one f16 rounding) plus what it inherits from the stage before (fp64_ref.propagate of
fp64_ref.mid_error) -- the error model of every fused conv chain of the suite, nothing added.

  stage 0  reflect-pad by k/2-1, depthwise k x k, stride 2, taps = dwt.taps32.to(dtype) (LL, LH, HL, HH)     K = k*k
  stage 1  (use_ds) depthwise 3x3, zero padding, no bias, on LH / HL / HH                                    K = 9
  stage 2  f_ll 1x1 on LL; f_h 3x3 (dense) or its pointwise 1x1 (use_ds) on each high band; bias, SiLU       K = c+1 / 9c+1 / c+1
  stage 3  Z = W_z . P (P = LL | LH | HL | HH processed, c/2 channels each), no bias, no activation          K = 2c

The Haar kernels multiply by float32(1/sqrt2)^2 = 0.49999997 where the f16 taps are 0.5: a relative 2^-24 inside the stage-0 bound."""
import torch
import torch.nn.functional as F

import fp64_ref as R


def wavelet_z_ref(x, taps, wl, bl, wh, bh, wz, wdw=None, f16_points=True):
    """x (B,c,H,W) with the values the kernel reads; taps (4,k,k) = dwt.taps32.to(dtype); wl (c/2,c,1,1), wh (c/2,c,3,3) or, with
    wdw (c,1,3,3) given (use_ds), the pointwise (c/2,c,1,1); wz (c,2c,1,1): weights as the kernel holds them (rounded to f16); bl, bh
    fp32 biases.  Returns (Z, bound, P, bound_P): Z (B,c,H/2,W/2) float64 and its per-element bound; P (B,2c,H/2,W/2) as stage 3
    reads it (rounded to f16) and the bound of an f16 P against it (mid_error of stage 2).  f16_points=False: nothing is rounded."""
    dev = x.device
    c, k = x.shape[1], taps.shape[-1]
    pad = k // 2 - 1
    x64 = x.to(torch.float64)
    xp = F.pad(x64, (pad, pad, pad, pad), mode="reflect") if pad else x64
    taps = taps.to(device=dev, dtype=torch.float64)
    P, eP = [], []
    for band in range(4):
        st = [R.stage(taps[band].expand(c, 1, k, k), None, k, 2, 0, dw=True, K=k * k)]
        if band == 0:
            st.append(R.stage(wl, bl, 1, 1, 0, R.ACT_SILU))
        else:
            if wdw is not None:
                st.append(R.stage(wdw, None, 3, 1, 1, dw=True, K=9))
                st.append(R.stage(wh, bh, 1, 1, 0, R.ACT_SILU))
            else:
                st.append(R.stage(wh, bh, 3, 1, 1, R.ACT_SILU))
        y, bnd = R.chain_ref([xp], st, f16_points=f16_points)
        mid = y.to(torch.float16).double() if f16_points else y
        P.append(mid)
        eP.append(R.mid_error(bnd, mid) if f16_points else bnd)
    P, eP = torch.cat(P, 1), torch.cat(eP, 1)
    z, A, Y = R.conv_ref([P], wz)
    bz = R.bound(z, A, Y, 2 * c) + R.propagate(eP, wz.to(dev), 1, 1, 0)
    return z, bz, P, eP


def enhancer_tail64(b, z, wb, bias, gamma_tanh):
    """The enhancer's tail in fp64: b + tanh(gamma) SiLU(W_b b + bilinear_up2x(Z) + bias) (resize_addz has the index arithmetic)."""
    y, _, _ = R.conv_ref([b.double()], wb, bias, 1, 1, 0, R.ACT_SILU, addz=z, out_scale=gamma_tanh, res=b.double())
    return y


# ---------------------------------------------------------------------------------------------------------------- data recipes
NAMES = {"haar": 2, "db2": 4, "db3": 6, "db4": 8}  # one bank per filter length the fused kernel is built for
CS = (16, 32, 64, 128)
MODEL_MAP = {16: 160, 32: 80, 64: 40, 128: 20}  # the enhancer's (c, map) pairs in yolo11-test.yaml at 640x640


def tile_h(c):
    return 4 if c == 128 else 8  # TH of wavelet_z_kernel (csrc/wavelet.hip, ey_wavelet_z2)


def bounded_shapes(name, c):
    """{kind: (B, H, W)} of the bounded cases of one instantiation: `ragged` = three tiles in x and in y with a ragged last one
    (half-resolution 18 x 34 against 16-wide, TH-high tiles), odd H and W, batch 3; `min` = the smallest legal map of the filter
    length (pad = H - 1; Haar: 2 rows), an odd width; `model` = the benchmarked model's own map for this c."""
    pad = NAMES[name] // 2 - 1
    return {"ragged": (3, 37, 69), "min": (3, max(pad + 1, 2), max(pad + 1, 2) + 1), "model": (2, MODEL_MAP[c], MODEL_MAP[c])}


# impulse maps, multi-tile (half-resolution 10 x 18): odd in both extents, and an even one -- a 4-tap bank reads no reflected row or
# column below / right of an odd map (its last window ends on the last pixel), so only an even map shows its lower reflection
IMPULSE_HWS = ((21, 37), (20, 36))

# Mean-ulp gates.  fp64_ref.report's project-wide gate is 0.5 ulp16, and every 4-, 6- and 8-tap instantiation meets it (0.19 .. 0.41).
# No Haar case but one does (1.1 .. 6.2): the Haar kernels (dwt_kernel and the fused kernel alike) multiply by float32(1/sqrt2)^2 =
# 0.49999997 where the reference's f16 taps are 0.5.  The sum of four f16 values times 0.5 sits EXACTLY on an f16 rounding boundary
# for 15% of the sub-band values of randn inputs (a tie: the reference rounds it to even, the kernel's value just below it rounds
# down), so 7.6% of the sub-band values differ from the reference by one ulp16, against ~1e-4 from fp32 summation order alone; each such ulp moves Z
# by |w| ulp16(sub-band) whatever |Z| is, which is many ulp16 of a Z near zero (Z has no bias and no activation and is centred on
# zero).  The per-element bound allows it (the relative 2^-24 of the taps is inside the stage-0 bound).  The unfused f16 path (dwt_kernel,
# the 4-group conv or f_ll + DSConvs, the 1x1 conv: each checked against fp64 on its own) has the same rounding points and the same
# taps.  Where a case does not meet 0.5, its gate is 1.25 x the mean ulp of the UNFUSED path on the same input against the same
# reference, measured on an MI355X and written here (the margin covers the different fp32 summation order of the fused MFMA loop;
# the fused kernel measured 0.999 .. 1.002 x these figures); never a figure of the fused kernel's own output.
# test_gpu_wavelet_exact re-measures every entry.  {f"{name}-{ds|conv}-C{c}-{kind}": measured unfused mean ulp}; step32 / step1 = the
# replays of the benchmarked forward's own calls at batch 32 / 1.
UNFUSED_MEAN_ULP = {
    "haar-conv-C16-ragged": 1.9676, "haar-conv-C16-model": 2.3756, "haar-conv-C32-ragged": 2.0905, "haar-conv-C32-min": 1.4362,
    "haar-conv-C32-model": 2.1398, "haar-conv-C64-ragged": 2.5091, "haar-conv-C64-min": 1.1410, "haar-conv-C64-model": 2.6022,
    "haar-conv-C128-ragged": 2.6070, "haar-conv-C128-min": 3.1563, "haar-conv-C128-model": 2.8340, "haar-ds-C16-ragged": 2.3922,
    "haar-ds-C16-min": 6.1793, "haar-ds-C16-model": 2.9496, "haar-ds-C32-ragged": 3.9392, "haar-ds-C32-min": 0.7713,
    "haar-ds-C32-model": 2.7857, "haar-ds-C64-ragged": 3.3181, "haar-ds-C64-min": 1.3297, "haar-ds-C64-model": 3.0037,
    "haar-ds-C128-ragged": 3.2616, "haar-ds-C128-min": 1.7365, "haar-ds-C128-model": 2.6224, "haar-conv-C16-step32": 2.4142,
    "haar-conv-C32-step32": 2.3997, "haar-conv-C64-step32": 2.4680, "haar-conv-C128-step32": 2.7892, "haar-conv-C16-step1": 2.2224,
    "haar-conv-C32-step1": 2.3527, "haar-conv-C64-step1": 2.4942, "haar-conv-C128-step1": 2.7350,
}


def case_id(name, use_ds, c, kind):
    return f"{name}-{'ds' if use_ds else 'conv'}-C{c}-{kind}"


def mean_ulp_gate(cid):
    return 1.25 * UNFUSED_MEAN_ULP[cid] if cid in UNFUSED_MEAN_ULP else 0.5


def weights(c, use_ds, gen):
    """General weights, scaled sqrt(2/K) like test_gpu_conv_exact._data and rounded to f16; biases 0.5 randn (fp32).
    Returns dict(wl, bl, wh, bh, wz, wdw) of float64 / fp32 CPU tensors (wdw None without use_ds)."""
    h = c // 2

    def w(shape, K):
        return (torch.randn(shape, generator=gen) * (2.0 / K) ** 0.5).half().double()

    d = dict(wl=w((h, c, 1, 1), c), bl=torch.randn(h, generator=gen).float() * 0.5)
    if use_ds:
        d.update(wdw=w((c, 1, 3, 3), 9), wh=w((h, c, 1, 1), c))
    else:
        d.update(wdw=None, wh=w((h, c, 3, 3), 9 * c))
    d.update(bh=torch.randn(h, generator=gen).float() * 0.5, wz=w((c, 2 * c, 1, 1), 2 * c))
    return d


def general_input(B, c, H, W, gen):
    return torch.randn((B, c, H, W), generator=gen).half().double()


def impulse_spots(H, W, TH):
    """Pixels (full resolution) of the impulse test: the four corners, both sides of the x tile seam (half-res x = 15 | 16) and of the
    y seam (half-res y = TH-1 | TH), the last row and the last column (of an odd map: unused by Haar, read through the reflection by
    longer banks), and the pixel next to each border (where reflect and zero padding differ).  Spots outside the map are dropped."""
    s = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),
         (5, 31), (5, 32), (H // 2, 30), (H // 2, 33),
         (2 * TH - 1, 7), (2 * TH, 7), (2 * TH - 2, W // 2), (2 * TH + 1, W // 2),
         (H - 1, W // 2), (H // 2, W - 1),
         (1, W // 3), (H - 2, W // 3), (H // 3, 1), (H // 3, W - 2), (1, 1), (H - 2, W - 2)]
    out = []
    for y, x in s:
        if 0 <= y < H and 0 <= x < W and (y, x) not in out:
            out.append((y, x))
    return out


def impulse_input(c, H, W, spots, gen):
    """One image per spot, zero except that pixel: all channels, f16 values in +-[1, 3]."""
    x = torch.zeros((len(spots), c, H, W), dtype=torch.float64)
    for i, (y, xx) in enumerate(spots):
        v = (1 + 2 * torch.rand(c, generator=gen)) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1)
        x[i, :, y, xx] = v.half().double()
    return x


def check_impulse(case, label, got0, got, z0, b0, z, bz, spots, H, W, k):
    """The impulse-locality assertions on a kernel (or emulation) output: got0 / got = Z of the all-zero image and of the impulse
    images, (z0, b0) / (z, bz) the references and bounds.  Outside the reference footprint (pixels where reference-Z(impulse) !=
    reference-Z(zero)) got must be bit-equal to the zero-input constant; inside it the bound holds; the zero-input Z is one constant
    vector within its bound; the footprint is non-empty except for the Haar impulses on the last row / column of an odd extent."""
    g0 = got0.to(device=z0.device, dtype=torch.float64)
    const = g0[0, :, 0, 0]
    assert bool((g0 == const.view(1, -1, 1, 1)).all()), f"{case} [{label}]: the zero-input Z is not one constant vector"
    assert bool(((g0 - z0).abs() <= b0).all()), f"{case} [{label}]: zero-input Z outside the bound"
    g = got.to(device=z.device, dtype=torch.float64)
    foot = (z != z0[:1]).any(1)  # (n, Ho, Wo)
    for i, (y, x) in enumerate(spots):
        unused = k == 2 and ((H % 2 and y == H - 1) or (W % 2 and x == W - 1))
        n = int(foot[i].sum())
        assert (n == 0) if unused else (n > 0), f"{case}: impulse at {(y, x)}: reference footprint of {n} pixels"
        off = (g[i] != const.view(-1, 1, 1)).any(0) & ~foot[i]
        if bool(off.any()):
            p = [int(v) for v in torch.nonzero(off)[0]]
            raise AssertionError(f"{case} [{label}]: impulse at {(y, x)} changes Z at half-res pixel {p}, outside the reference footprint "
                                 f"({int(off.sum())} such pixels)")
        bad = (g[i] - z[i]).abs() > bz[i]
        if bool(bad.any()):
            p = [int(v) for v in torch.nonzero(bad)[0]]
            raise AssertionError(f"{case} [{label}]: impulse at {(y, x)}: {int(bad.sum())} elements exceed the bound, first (c,y,x)={p}: "
                                 f"got {float(g[i][tuple(p)])} want {float(z[i][tuple(p)])} bound {float(bz[i][tuple(p)]):.3g}")
    print(f"[impulse] {case} [{label}] {len(spots)} impulses local and within the bound")
