"""float64 restatements for the pose task, written from the formulas (keypoint anchor decode, object keypoint similarity): the yardstick
the HIP kernels and the reference's fp32 results are both measured against.  numpy."""
import numpy as np

EPS = 1e-7


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def decode(levels, strides, kpt_shape, dtype=np.float64):
    """levels: per level keypoint logits (B, nk, H, W) -> (B, nk, A) of `dtype`: channel (k, 0) = (v * 2 + gx) * stride, (k, 1) = (v * 2 + gy) *
    stride, (k, 2) = sigmoid(v); gx, gy the anchor's grid cell.  dtype=np.float32 is the fp32 evaluation, one rounding per x / y value."""
    ndim = kpt_shape[1]
    out = []
    for kp, s in zip(levels, strides):
        kp = np.asarray(kp, dtype)
        B, nk, H, W = kp.shape
        v = kp.reshape(B, nk, H * W)
        gx, gy = np.tile(np.arange(W), H).astype(dtype), np.repeat(np.arange(H), W).astype(dtype)
        y = np.empty_like(v)
        y[:, 0::ndim] = (v[:, 0::ndim] * dtype(2) + gx) * dtype(s)
        y[:, 1::ndim] = (v[:, 1::ndim] * dtype(2) + gy) * dtype(s)
        if ndim == 3:
            y[:, 2::3] = _sigmoid(v[:, 2::3].astype(np.float64)).astype(dtype)
        out.append(y)
    return np.concatenate(out, 2)


def kpt_iou64(gt, pred, area, sigma):
    """gt (M,K,3), pred (N,K,>=2), area (M,), sigma (K,) -> (M,N) float64: the mean over the visible keypoints of
    exp(-d^2 / (2 (2 sigma)^2 (area + eps))); 0 for a ground truth without a visible keypoint."""
    gt, pred, area, sigma = (np.asarray(t, np.float64) for t in (gt, pred, area, sigma))
    d = (gt[:, None, :, 0] - pred[None, :, :, 0]) ** 2 + (gt[:, None, :, 1] - pred[None, :, :, 1]) ** 2
    vis = gt[..., 2] != 0
    e = d / ((2 * sigma) ** 2 * (area[:, None, None] + EPS) * 2)
    return (np.exp(-e) * vis[:, None]).sum(-1) / (vis.sum(-1)[:, None] + EPS)


def box_iou64(b1, b2):
    b1, b2 = np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    lt, rb = np.maximum(b1[:, None, :2], b2[None, :, :2]), np.minimum(b1[:, None, 2:], b2[None, :, 2:])
    inter = np.clip(rb - lt, 0, None).prod(2)
    a1, a2 = (b1[:, 2:] - b1[:, :2]).prod(1), (b2[:, 2:] - b2[:, :2]).prod(1)
    return inter / (a1[:, None] + a2[None] - inter + EPS)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def bound(err_ref, value):
    """The tolerance rule for every float output of the pose kernels: 4 E + 2 ulp(fp32) of the value, E = the reference's own fp32 error."""
    return 4.0 * err_ref + 2.0 * ulp32(value)
