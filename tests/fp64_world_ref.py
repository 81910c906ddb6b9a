"""float64 restatements for the YOLO-World tests: the max-sigmoid attention gate (reference nn/modules/block.py:558-576 behind `gl` and
`proj_conv`) and the unfolded contrastive class tail of WorldDetect (BNContrastiveHead, block.py:687-692, on the tower's closing 1x1 conv).
numpy only."""
import numpy as np

SQRT_HC = float(np.float32(32 ** 0.5))  # the reference divides by the python float 32**0.5; torch rounds the scalar to the tensor's fp32


def max_sigmoid_attn64(e, p, g, bias, scale=None, nh=None):
    """e, p (B, C, H, W); g (Bg, n, C) with Bg = 1 or B; bias (nh,); scale (nh,) or None -> (y (B, C, H, W), score (B, nh, H, W) the
    maximum dot per pixel and head, before the division), all float64."""
    e, p, g = np.asarray(e, np.float64), np.asarray(p, np.float64), np.asarray(g, np.float64)
    B, C, H, W = e.shape
    nh = len(bias) if nh is None else nh
    hc = C // nh
    if g.shape[0] == 1:
        g = np.broadcast_to(g, (B,) + g.shape[1:])
    ee = e.reshape(B, nh, hc, H, W)
    gg = g.reshape(B, -1, nh, hc)
    s = np.einsum("bmchw,bnmc->bmhwn", ee, gg).max(-1)
    a = s / SQRT_HC + np.asarray(bias, np.float64)[None, :, None, None]
    aw = 1.0 / (1.0 + np.exp(-a))
    if scale is not None:
        aw = aw * np.asarray(scale, np.float64)[None, :, None, None]
    return (p.reshape(B, nh, hc, H, W) * aw[:, :, None]).reshape(B, C, H, W), s


def contrastive_tail64(h, w3, b3, bn_w, bn_b, bn_mean, bn_var, eps, txt, logit_scale, bias):
    """The unfolded class tail in float64: h (B, c3, H, W) tower activations -> logits (B, n, H, W) =
    exp(logit_scale) * <BatchNorm(W3 h + b3), normalize(txt)> + bias."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    x = np.einsum("oc,bchw->bohw", f(w3).reshape(len(f(b3)), -1), f(h)) + f(b3)[None, :, None, None]
    x = (x - f(bn_mean)[None, :, None, None]) / np.sqrt(f(bn_var)[None, :, None, None] + eps) * f(bn_w)[None, :, None, None] + f(bn_b)[None, :, None, None]
    t = f(txt).reshape(-1, f(txt).shape[-1])
    t = t / np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-12)
    return np.einsum("bchw,kc->bkhw", x, t) * np.exp(float(f(logit_scale))) + float(f(bias).reshape(-1)[0])


def apply_fold64(h, w, b):
    """The folded tail applied in float64: (n, c3[, 1, 1]) weight and (n,) bias on h (B, c3, H, W)."""
    w = np.asarray(w, np.float64).reshape(len(b), -1)
    return np.einsum("kc,bchw->bkhw", w, np.asarray(h, np.float64)) + np.asarray(b, np.float64)[None, :, None, None]
