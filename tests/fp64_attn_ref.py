"""fp64 references of the attention cores (ey_linear_attention, ey_softmax_attention, the EY_BLK_LINATTN block stage) and of the
head decode (head_decode_kernel), with per-element error bounds derived from the kernels' arithmetic.

Notation: U = 2^-24 is the fp32 unit roundoff; a sum of K fp32 terms in any order is within K*U*sum|terms| of the exact sum
(the usual gamma_K bound; the factor 1.01 below absorbs the second-order terms).  The constants rest on the ISA's documented accuracy:

* v_exp_f32 and v_rcp_f32 are accurate to 1 ulp; EXP_REL = RCP_REL = 2^-22 (2 ulp) covers either.  `__expf(x)` is
  v_exp_f32(x * log2(e)): the argument x = a - m is rounded once (U|x|), the multiply once, and log2(e) itself is an fp32
  constant, so the argument carries a relative error of 3U; the softmax-attention MFMA kernel rounds once more ((S - m) * scale),
  so ARG_REL = 4U is used everywhere.  An argument error dx becomes a relative error dx of the exponential.
* `1.f / x` (IEEE division) is within RCP_REL too.
* Values below 2^-126 (exp underflow into subnormals or to 0, sigmoid(x) for x < -88 where exp(-x) overflows) carry an absolute
  error of at most TINY = 2^-126.

Softmax rows (`softmax_terms`): the kernel evaluates e_m = exp(a_m - mx) with its own fp32 logits a_m = z_m + eps_m
(|eps_m| <= dz_m) and its own fp32 max mx.  mx is one fp32 number shared by every term, so it cancels in e_m / sum(e); hence
    P_kernel_m = P_m * (1 + eps_m + eta_m) / sum_k P_k (1 + eps_k + eta_k),   eta_m = ARG_REL |z_m - max z| + EXP_REL,
and with r_m = dz_m + eta_m, r_bar = sum_k P_k r_k the relative error of P_m is at most
    1.01 (r_m + r_bar + (K + 1) U + RCP_REL)
for K summed terms (the fp32 sum of e, the rcp / division, the multiply e * inv).

A contraction y = sum_m P_m v_m of K terms then errs by sum_m dP_m |v_m| + (K + 2) U sum_m P_m |v_m| (fp32 accumulation,
one product rounding).  At an intermediate f16 rounding point t16 = f16(t) a kernel value within dt of the exact t may round to
the neighbouring f16, so the rounded intermediate errs by dt + ulp16(t16) against f16 of the fp64 value (`_round16`, the
`mid_error` of fp64_ref); the reference rounds there too and the next contraction propagates the sum.  The outputs get one final
rounding (`out_bound`): ulp16 of the value in f16, ulp32 in f32.

Every reference returns (y, E, Y): the fp64 result with the intermediate roundings of the kernel path it checks, E, the bound on
the error of the kernel's fp32 value before its output rounding, and Y >= |y|, the magnitude of the terms of the last operation
(sum |qs||ctx|, sum P|v|, the box corner terms): fp32 outputs that cancel (y near 0 with Y large) are graded in ulp32(Y) by
`report32`, since their error scales with Y, not with |y|."""
import numpy as np
import torch

from fp64_ref import ulp16

U = 2.0 ** -24
EXP_REL = 2.0 ** -22
RCP_REL = 2.0 ** -22
ARG_REL = 4 * U
TINY = 2.0 ** -126
Q_LO = float(np.float32(1e-6))                               # clamp(q, 1e-6f, 1.f - 1e-6f) of the kernel, in fp32
Q_HI = float(np.float32(1.0) - np.float32(1e-6))


def ulp32(v):
    """np.spacing of the fp32 value of v (the gap above |f32(v)|) as float64: 2^(e-23), subnormal floor 2^-149."""
    h = v.to(torch.float32).abs().double()
    e = torch.floor(torch.log2(h.clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


def out_bound(y, E, dtype):
    """E (error of the kernel's fp32 value) + one output rounding to `dtype`."""
    return E + (ulp16(y) if dtype == torch.float16 else ulp32(y))


def softmax_terms(z, dim, dz=None):
    """Exact softmax P of logits z along dim and the bound dP on |P_kernel - P| (module docstring).  dz: bound on the error of
    the kernel's logits (None: the logits are the exact inputs)."""
    K = z.shape[dim]
    x = z - z.amax(dim, keepdim=True)
    e = torch.exp(x)
    P = e / e.sum(dim, keepdim=True)
    r = ARG_REL * x.abs() + EXP_REL
    if dz is not None:
        r = r + dz * (1 + ARG_REL)
    rbar = (P * r).sum(dim, keepdim=True)
    rel = 1.01 * (r + rbar + (K + 1) * U + RCP_REL)
    return P, P * rel + TINY


def _round16(t, dt):
    """f16 rounding point: (f16(t), bound of the kernel's rounded value against it)."""
    t16 = t.to(torch.float16).double()
    return t16, dt + ulp16(t16)


def _rows(x):
    """logical-NCHW tensor (any dtype, any view) -> (B, N, C) float64 on its device."""
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C).double()


def linear_attention_ref(qkv, heads, f16_points=False):
    """LinearAttention core: ks = softmax over head_dim of k, qs = softmax over the N pixels of q, ctx = ks^T v, y = qs ctx, per
    (image, head), in float64.  f16_points: ks, ctx and qs rounded to f16 where the MFMA kernel (and the block stage) rounds them;
    otherwise fp32 throughout (the VALU kernel).  qkv: logical (B, 3C, H, W) with channels [q | k | v].  Returns (y (B, N, C), E,
    Y = qs |ctx|).

    Bound: dks from the softmax over d (K = d terms); ctx errs by dks^T |v| + (N + 2) U ks^T |v|; dqs from the softmax over N;
    y errs by dqs (|ctx| + Ectx) + qs Ectx + (d + 2) U qs |ctx| -- with the f16 neighbour term added at ks, ctx and qs when
    f16_points."""
    t = _rows(qkv)
    B, N, C3 = t.shape
    C = C3 // 3
    d = C // heads
    q, k, v = (t[..., i * C:(i + 1) * C].reshape(B, N, heads, d).transpose(1, 2) for i in range(3))  # (B, heads, N, d)
    ks, dks = softmax_terms(k, -1)
    qs, dqs = softmax_terms(q, -2)
    if f16_points:
        ks, dks = _round16(ks, dks)
        qs, dqs = _round16(qs, dqs)
    va = v.abs()
    ctx = ks.transpose(-1, -2) @ v
    Ectx = dks.transpose(-1, -2) @ va + (N + 2) * U * (ks.transpose(-1, -2) @ va)
    if f16_points:
        ctx, Ectx = _round16(ctx, Ectx)
    ca = ctx.abs()
    y = qs @ ctx
    E = dqs @ (ca + Ectx) + qs @ Ectx + (d + 2) * U * (qs @ ca)
    return tuple(t.transpose(1, 2).reshape(B, N, C) for t in (y, E, qs @ ca))


def softmax_attention_ref(qkv, heads, kd, hd, scale, f16_points=False):
    """Attention core: per (image, head) with channels [q (kd) | k (kd) | v (hd)], P = softmax over keys m of scale * q_n . k_m,
    y_n = sum_m P[n, m] v_m, in float64.  f16_points: P rounded to f16 (the MFMA kernel: P = f16(e * rcp(sum))); otherwise fp32
    throughout (the VALU kernel).  Returns (y (B, N, heads * hd), E, Y = P |v|).

    Bound: the fp32 score of kd exact products errs by (kd + 2) U scale |q||k| (the VALU kernel rounds q * scale first; the MFMA
    kernel scales after the max subtraction, covered by ARG_REL); softmax_terms over the N keys; y errs by dP |v| + (N + 2) U P |v|."""
    t = _rows(qkv)
    B, N, _ = t.shape
    per = 2 * kd + hd
    t = t[..., :heads * per].reshape(B, N, heads, per).transpose(1, 2)  # (B, heads, N, per)
    q, k, v = t[..., :kd], t[..., kd:2 * kd], t[..., 2 * kd:]
    S = scale * (q @ k.transpose(-1, -2))
    dS = (kd + 2) * U * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2))
    P, dP = softmax_terms(S, -1, dS)
    if f16_points:
        P, dP = _round16(P, dP)
    va = v.abs()
    y = P @ v
    Y = P @ va
    E = dP @ va + (N + 2) * U * Y
    return tuple(t.transpose(1, 2).reshape(B, N, heads * hd) for t in (y, E, Y))


def _sigmoid_terms(x):
    """sigmoid(x) = rcp(1 + __expf(-x)) in fp32: exact value and the bound of the kernel's error (exp argument 2U|x| + EXP_REL,
    relative weight 1 - s; the add; the rcp)."""
    s = torch.sigmoid(x)
    return s, s * ((1 - s) * (2 * U * x.abs() + EXP_REL) + U + RCP_REL) + TINY


def head_decode_ref(levels, nc, A_total, xyxy=False):
    """head_decode_kernel in float64: per anchor 4 x softmax(16) of the box logits, DFL expectation, top-4 + mean of each side,
    quality q = clamp(sigmoid(FC(64->1)(ReLU(FC(20->64)(stats)))), 1e-6f, 1 - 1e-6f) (1 without a quality head), box decode
    around (x + 0.5, y + 0.5) times the stride, scores sigmoid(cls) * q.  levels: list of (box (B,64,H,W), cls (B,nc,H,W), stride,
    q = (w1 [hid,20], b1, w2 [hid], b2) or None, a_off).  No intermediate rounding: the kernel is fp32 throughout and writes fp32.
    Returns (pred (B, 4+nc, A_total) with NaN in columns no level covers, E (same shape, 0 there), Y (stride (x + 0.5 + dist terms)
    for the box rows, |score| for the scores)).

    Bound (the file is compiled without FMA contraction): dist = sum_i i P_i errs by sum_i i dP_i + 18 U sum_i i P_i; a sorted
    top-4 entry by at most max_i dP_i (order statistics of perturbed values); the mean by (sum dP + 16 U) / 16.  The hidden layer by
    |w1| dstat + 12 U (|b1| + |w1||stat|) (ReLU is 1-Lipschitz), o by |w2| dh + (hid + 2) U (|b2| + |w2||h|); q by o's error / 4
    (sigmoid' <= 1/4) + the sigmoid's own (_sigmoid_terms); the clamp is 1-Lipschitz.  A box row errs by stride (its dist errors
    (halved for the centre) + 4 U (x + 0.5 + dist terms)); a score by dsig q + sig dq + U sig q."""
    box0 = levels[0][0]
    B = box0.shape[0]
    dev = box0.device
    pred = torch.full((B, 4 + nc, A_total), float("nan"), dtype=torch.float64, device=dev)
    E = torch.zeros_like(pred)
    Y = torch.zeros_like(pred)
    bins = torch.arange(16, dtype=torch.float64, device=dev)
    for box, cls, stride, qh, a_off in levels:
        _, _, H, W = box.shape
        HW = H * W
        lg = _rows(box).reshape(B, HW, 4, 16)
        P, dP = softmax_terms(lg, -1)
        dist = (P * bins).sum(-1)                                             # (B, HW, 4)
        Ed = (dP * bins).sum(-1) + 18 * U * dist
        if qh is not None:
            w1, b1, w2, b2 = (t.to(device=dev, dtype=torch.float64) for t in qh)
            top = P.sort(-1, descending=True).values[..., :4]
            mean = P.sum(-1, keepdim=True) / 16
            stat = torch.cat([top, mean], -1).reshape(B, HW, 20)
            dmax = dP.amax(-1, keepdim=True)
            Emean = (dP.sum(-1, keepdim=True) + 16 * U * P.sum(-1, keepdim=True)) / 16
            Estat = torch.cat([dmax.expand(-1, -1, -1, 4), Emean], -1).reshape(B, HW, 20)
            hp = stat @ w1.T + b1
            Eh = Estat @ w1.abs().T + 12 * U * (b1.abs() + stat.abs() @ w1.abs().T)
            h = hp.clamp_min(0)
            o = h @ w2 + b2
            Eo = Eh @ w2.abs() + (w2.numel() + 2) * U * (b2.abs() + h @ w2.abs())
            s, Es = _sigmoid_terms(o)
            q = s.clamp(Q_LO, Q_HI)
            Eq = 0.25 * Eo + Es
        else:
            q = torch.ones((B, HW), dtype=torch.float64, device=dev)
            Eq = torch.zeros_like(q)
        a = torch.arange(HW, device=dev)
        cx0 = (a % W).double() + 0.5
        cy0 = torch.div(a, W, rounding_mode="floor").double() + 0.5
        d0, d1, d2, d3 = dist.unbind(-1)
        e0, e1, e2, e3 = Ed.unbind(-1)
        x1, y1, x2, y2 = cx0 - d0, cy0 - d1, cx0 + d2, cy0 + d3
        mx, my = cx0 + d0 + d2, cy0 + d1 + d3
        if xyxy:
            rows = [x1, y1, x2, y2]
            err = [e0 + 4 * U * mx, e1 + 4 * U * my, e2 + 4 * U * mx, e3 + 4 * U * my]
        else:
            rows = [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1]
            err = [(e0 + e2) / 2 + 4 * U * mx, (e1 + e3) / 2 + 4 * U * my, e0 + e2 + 4 * U * mx, e1 + e3 + 4 * U * my]
        cols = slice(a_off, a_off + HW)
        for r in range(4):
            pred[:, r, cols] = rows[r] * stride
            E[:, r, cols] = err[r] * stride
            Y[:, r, cols] = (mx if r % 2 == 0 else my) * stride
        sig, Esig = _sigmoid_terms(_rows(cls))                                  # (B, HW, nc)
        sc = sig * q.unsqueeze(-1)
        Esc = Esig * q.unsqueeze(-1) + sig * Eq.unsqueeze(-1) + U * sc
        pred[:, 4:, cols] = sc.transpose(1, 2)
        E[:, 4:, cols] = Esc.transpose(1, 2)
        Y[:, 4:, cols] = sc.transpose(1, 2)
    return pred, E, Y


def report32(case, label, got, y, bnd, Y, mean_ulp_max):
    """fp32-output counterpart of fp64_ref.report: per-element bound + a gate on the mean of |err| / ulp32(Y) (Y: the magnitude
    the reference returns).  Returns (max err/bound, mean ulp)."""
    g = got.to(device=y.device, dtype=torch.float64)
    assert torch.isfinite(g).all(), f"{case} [{label}]: non-finite output"
    err = (g - y).abs()
    mu = float((err / ulp32(torch.maximum(Y, y.abs()))).mean())
    rb = float((err / bnd).max())
    print(f"[fp64] {case} [{label}] max err/bound {rb:.3f}  mean ulp32 {mu:.3f}  max |y| {float(y.abs().max()):.3g}")
    bad = err > bnd
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{case} [{label}]: {int(bad.sum())} elements exceed the fp64 bound (max err/bound {rb:.3f}); first at flat index {i}: "
                             f"got {float(g.flatten()[i])} want {float(y.flatten()[i])} bound {float(bnd.flatten()[i]):.3g}")
    assert mu <= mean_ulp_max, f"{case} [{label}]: mean error {mu:.3f} ulp32 > {mean_ulp_max}"
    return rb, mu
