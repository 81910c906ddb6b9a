"""Restatements for the YOLOv9 (GELAN) tests, numpy only: the ADown / AConv pooling front end (reference nn/modules/block.py:753-784), CBFuse
(:821-833) and the RepConv fold (nn/modules/conv.py:228-269) -- in float64, and, for the two kernels, in the stated fp32 operation order with
one rounding to the storage type (what ey_adown_pool and ey_cbfuse promise bit for bit)."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------- adown_pool
def _windows(x):
    return x[:, :, :-1, :-1], x[:, :, :-1, 1:], x[:, :, 1:, :-1], x[:, :, 1:, 1:]


def _maxpool3s2p1(a):
    """max_pool2d(a, 3, 2, 1) on (B, C, Ha, Wa): window positions outside the map are skipped."""
    B, C, Ha, Wa = a.shape
    Hm, Wm = (Ha - 1) // 2 + 1, (Wa - 1) // 2 + 1
    out = np.empty((B, C, Hm, Wm), a.dtype)
    for j in range(Hm):
        for q in range(Wm):
            out[:, :, j, q] = a[:, :, max(2 * j - 1, 0):min(2 * j + 2, Ha), max(2 * q - 1, 0):min(2 * q + 2, Wa)].max(axis=(2, 3))
    return out


def adown_pool64(x, c_avg):
    """float64: a = avg_pool2d(x, 2, 1, 0)[:, :c_avg], m = max_pool2d(avg[:, c_avg:], 3, 2, 1) (None when c_avg == C)."""
    x = np.asarray(x, np.float64)
    x00, x01, x10, x11 = _windows(x)
    A = (x00 + x01 + x10 + x11) * 0.25
    return A[:, :c_avg], (_maxpool3s2p1(A[:, c_avg:]) if c_avg < x.shape[1] else None)


def adown_pool_stated(x, c_avg, dtype):
    """The stated order: fp32 ((x00 + x01) + x10) + x11, times 0.25f, rounded once to `dtype`; the maximum over the ROUNDED values."""
    x = np.asarray(x).astype(dtype).astype(np.float32)
    x00, x01, x10, x11 = _windows(x)
    A = ((((x00 + x01) + x10) + x11) * np.float32(0.25)).astype(dtype)
    return A[:, :c_avg], (_maxpool3s2p1(A[:, c_avg:]) if c_avg < x.shape[1] else None)


# ---------------------------------------------------------------------------------------------------------------- cbfuse
def nearest_index(n_out, n_in):
    """PyTorch's mode="nearest" source index for every destination index: min((int)floorf(dst * ((float)in / (float)out)), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def _resized(srcs):
    H, W = srcs[-1].shape[2:]
    return [np.asarray(s)[:, :, nearest_index(H, s.shape[2])][:, :, :, nearest_index(W, s.shape[3])] for s in srcs]


def cbfuse64(srcs):
    """float64 sum of the sources resized to the last one's size -> (sum, sum of absolute terms)."""
    t = [r.astype(np.float64) for r in _resized(srcs)]
    return sum(t), sum(np.abs(v) for v in t)


def cbfuse_stated(srcs, dtype):
    """The stated order: fp32 sum in list order starting from source 0, one rounding to `dtype`."""
    t = [r.astype(dtype).astype(np.float32) for r in _resized(srcs)]
    acc = t[0]
    for v in t[1:]:
        acc = acc + v
    return acc.astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- RepConv
def repconv_branches64(sd, eps, prefix=""):
    """The branches of an unfused RepConv state_dict {conv1.conv.weight, conv1.bn.*, conv2.conv.weight, conv2.bn.*[, bn.*]} (values: arrays),
    each with its BatchNorm (epsilon `eps`) folded in float64 and written as a 3x3 kernel: [(kernel (c2, c1, 3, 3), bias (c2,)), ...] for
    conv1, conv2 (zero-padded 1x1) and, when present, the identity BatchNorm."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items() if not k.endswith("num_batches_tracked")}

    def bn(p):
        s = sd[p + "weight"] / np.sqrt(sd[p + "running_var"] + eps)
        return s, sd[p + "bias"] - sd[p + "running_mean"] * s

    s3, b3 = bn(prefix + "conv1.bn.")
    s1, b1 = bn(prefix + "conv2.bn.")
    k3 = sd[prefix + "conv1.conv.weight"] * s3[:, None, None, None]
    k1 = np.zeros_like(k3)
    k1[:, :, 1:2, 1:2] = sd[prefix + "conv2.conv.weight"] * s1[:, None, None, None]
    out = [(k3, b3), (k1, b1)]
    if prefix + "bn.weight" in sd:
        sid, bid = bn(prefix + "bn.")
        kid = np.zeros_like(k3)
        kid[np.arange(len(sid)), np.arange(len(sid)), 1, 1] = sid
        out.append((kid, bid))
    return out


def repconv_fold64(sd, eps, prefix=""):
    """get_equivalent_kernel_bias in float64: the sum of the branches -> (3x3 kernel (c2, c1, 3, 3), bias (c2,))."""
    br = repconv_branches64(sd, eps, prefix)
    return sum(k for k, _ in br), sum(b for _, b in br)


def conv3x3_64(x, k, b):
    """3x3 stride-1 pad-1 convolution in float64: x (B, c1, H, W), k (c2, c1, 3, 3), b (c2,)."""
    x = np.asarray(x, np.float64)
    B, _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((B, k.shape[0], H, W))
    for dy in range(3):
        for dx in range(3):
            y += np.einsum("oc,bchw->bohw", k[:, :, dy, dx], xp[:, :, dy:dy + H, dx:dx + W])
    return y + b[None, :, None, None]


def silu64(v):
    return v / (1.0 + np.exp(-v))
