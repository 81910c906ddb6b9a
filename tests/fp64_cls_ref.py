"""float64 restatements of the classify kernels (csrc/classify.hip), numpy only: the conv + SiLU + mean of ey_classify_pool with the
magnitudes its error bound needs, linear + softmax of ey_classify_linear_softmax with the ranking rule, and the resize + crop of
ey_classify_transform (Pillow's antialiased bilinear coefficients, both axes, no intermediate rounding)."""
import numpy as np


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def bound(err_ref, value):
    """4 E + 2 ulp(fp32) of the value, E = the reference's own fp32 error (the rule of tests/fp64_obb_ref.py)."""
    return 4.0 * err_ref + 2.0 * ulp32(value)


# ---------------------------------------------------------------------------------------------------------------- ey_classify_pool
def pool64(x, w, b, silu):
    """x (B, C1, H, W), w (Cout, C1), b (Cout,) -> (mean (B, Cout), A (B, Cout), Y (B, Cout)) in float64: A = mean over the pixels of
    sum_k |x w| + |b| (what the accumulation error scales with), Y = mean over the pixels of |activated value|."""
    x, w, b = (np.asarray(t, np.float64) for t in (x, w, b))
    B, C1 = x.shape[:2]
    xp = x.reshape(B, C1, -1)
    pre = np.einsum("bkp,ok->bop", xp, w) + b[None, :, None]
    mag = np.einsum("bkp,ok->bop", np.abs(xp), np.abs(w)) + np.abs(b)[None, :, None]
    act = pre / (1.0 + np.exp(-pre)) if silu else pre
    return act.mean(2), mag.mean(2), np.abs(act).mean(2)


def pool_bound(A, Y, K, HW):
    """|got - mean| <= 1.1 K 2^-23 A + 2^-20 Y + (HW + 2) 2^-24 Y.  First term: fp32 accumulation of K products and the bias in any order,
    through SiLU (slope <= 1.1), the rule of tests/fp64_ref.bound, averaged over the pixels.  Second: the activation itself -- the fast
    exponential and the hardware reciprocal of the conv kernels' SiLU, a few fp32 ulp of every activated value (2^-20 = 8 ulp).  Third: the
    fp32 sum of HW activated values in any order, and the division."""
    return 1.1 * K * 2.0 ** -23 * A + 2.0 ** -20 * Y + (HW + 2) * 2.0 ** -24 * Y


# ---------------------------------------------------------------------------------------------------------------- linear + softmax + top-k
def linear_softmax64(pooled, w, b):
    pooled, w, b = (np.asarray(t, np.float64) for t in (pooled, w, b))
    logits = pooled @ w.T + b
    e = np.exp(logits - logits.max(1, keepdims=True))
    return logits, e / e.sum(1, keepdims=True)


def rank(probs, k=5):
    """descending probability, equal probabilities by ascending class index -> (B, min(nc, k)) int32."""
    p = np.asarray(probs)
    return np.argsort(-p, axis=1, kind="stable")[:, :min(p.shape[1], k)].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- resize + crop
def coeffs(insz, outsz, dtype=np.float64):
    """Pillow's antialiased BILINEAR coefficients as an (outsz, insz) matrix: scale = in / out, fs = max(scale, 1), center = (i + 0.5) scale,
    taps [max(int(center - fs + 0.5), 0), min(int(center + fs + 0.5), in)), weight max(0, 1 - |(x - center + 0.5) / fs|) normalised to sum 1."""
    scale = insz / outsz
    fs = max(scale, 1.0)
    M = np.zeros((outsz, insz), np.float64)
    for i in range(outsz):
        c = (i + 0.5) * scale
        lo, hi = max(int(c - fs + 0.5), 0), min(int(c + fs + 0.5), insz)
        xs = np.arange(lo, hi)
        wt = np.maximum(0.0, 1.0 - np.abs((xs - c + 0.5) / fs))
        M[i, xs] = wt / wt.sum()
    return M.astype(dtype)


def resized(h, w, S):
    return (int(S * h / w), S) if w <= h else (S, int(S * w / h))


def crop_origin(n, S):
    return int(round((n - S) / 2.0))


def transform(img, S, dtype=np.float64):
    """img (h, w, 3) uint8 -> (S, S, 3) grey levels 0..255 in `dtype` (same channel order): Resize(S) then CenterCrop(S), evaluated in
    `dtype` (the coefficients are computed in float64 and rounded to it), rows first then columns like the kernel."""
    h, w = img.shape[:2]
    nh, nw = resized(h, w, S)
    t, l = crop_origin(nh, S), crop_origin(nw, S)
    V, H = coeffs(h, nh, dtype)[t:t + S], coeffs(w, nw, dtype)[l:l + S]
    f = np.einsum("xw,hwc->hxc", H, img.astype(dtype))
    return np.einsum("yh,hxc->yxc", V, f)


def to_tensor(levels, dtype=np.float64):
    """(S, S, 3) grey levels -> (3, S, S) in [0, 1] (ToTensor)."""
    return (np.asarray(levels, dtype) / dtype(255.0)).transpose(2, 0, 1)
