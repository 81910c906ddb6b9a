"""fp64 reference of the MFMA conv operator (im2col + matmul in float64, on the tensor's device) and the per-element error
bounds of the f16 kernels derived from their arithmetic.

Every f16 conv kernel accumulates exact f16 x f16 products in fp32 (MFMA f32_16x16x32_f16, v_fma_mix_f32), adds the fp32 bias,
applies the activation in fp32 and rounds once to f16.  Hence:

* on small dyadic data (integer inputs, weights in multiples of 1/4, ...) every partial sum is exact in fp32 whatever the
  summation order, and the output must be BIT-IDENTICAL to the fp64 reference (`assert_exact`);
* on general data a per-element bound follows from the arithmetic (`bound`): fp32 accumulation of K terms in any order,
  the fp32 SiLU (__expf + rcp, a few ulp32, slope <= 1.1) and one f16 output rounding.

The reference is plain `F.unfold` + `@` in torch.float64 (rocBLAS dgemm on the GPU), chunked by image so that the
benchmark shapes (batch 32 at 640x640) fit; it never calls F.conv2d in float64."""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2
_CHUNK_BYTES = 256 << 20  # fp64 im2col columns per chunk


def ulp16(v):
    """np.spacing of the f16 value of v (the gap above |f16(v)|), as float64: 2^(e-10), subnormal floor 2^-24."""
    h = v.to(torch.float16).abs().double()
    e = torch.floor(torch.log2(h.clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def _src64(t, up, dev):
    t = t.to(device=dev, dtype=torch.float64)
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3) if up else t


def _act(v, act):
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    if act == ACT_RELU:
        return v.clamp_min(0)
    assert act == ACT_NONE, act
    return v


def resize_addz(z, Ho, Wo):
    """F.interpolate(z, (Ho, Wo), bilinear, align_corners=False) in fp64 with the index arithmetic of the conv epilogue
    (ATen area_pixel_compute_source_index, scale = in / out).  Returns (resized z, resized |z|)."""
    B, C, Hz, Wz = z.shape

    def idx(n_out, n_in, dev):
        s = ((torch.arange(n_out, device=dev, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
        i0 = s.floor().long()
        i1 = (i0 + 1).clamp_max(n_in - 1)
        l1 = s - i0
        return i0, i1, 1 - l1, l1

    y0, y1, ly0, ly1 = idx(Ho, Hz, z.device)
    x0, x1, lx0, lx1 = idx(Wo, Wz, z.device)
    out = []
    for t in (z, z.abs()):
        r0, r1 = t[:, :, y0], t[:, :, y1]
        rows = r0 * ly0.view(1, 1, -1, 1) + r1 * ly1.view(1, 1, -1, 1)
        out.append(rows[..., x0] * lx0 + rows[..., x1] * lx1)
    return out


def conv_ref(srcs, w, b=None, k=1, s=1, p=0, act=ACT_NONE, up=None, addz=None, out_scale=1.0, res=None, device=None):
    """y = res + out_scale * act(conv(cat(up2x?(srcs)), w) + b + bilinear(addz)) in float64, the semantics of nn._ops.conv2d
    for one group.  srcs: 1-2 logical-NCHW tensors (any strides); w (Cout, Cin, k, k) -- pass the values the kernel sees (for
    f16, the weights rounded to f16); b fp32 (Cout,).  Returns (y, A, Y):
      A = sum |w x| + |b| + |addz| (the same contraction on absolute values, before the activation),
      Y = |out_scale * act(v)| + |res| (magnitude of the terms of the final fp32 sum)."""
    dev = device or srcs[0].device
    up = up or [0] * len(srcs)
    B = srcs[0].shape[0]
    H, W = srcs[0].shape[2] << up[0], srcs[0].shape[3] << up[0]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    cin = sum(t.shape[1] for t in srcs)
    wm = w.to(device=dev, dtype=torch.float64).reshape(w.shape[0], -1)
    assert wm.shape[1] == cin * k * k, (tuple(w.shape), cin, k)
    wa = wm.abs()
    cout = wm.shape[0]
    per_img = cin * k * k * Ho * Wo * 8
    cb = max(1, min(B, _CHUNK_BYTES // max(per_img, 1)))
    y = torch.empty((B, cout, Ho, Wo), dtype=torch.float64, device=dev)
    A = torch.empty_like(y)
    for i in range(0, B, cb):
        x = torch.cat([_src64(t[i:i + cb], u, dev) for t, u in zip(srcs, up)], 1)
        cols = F.unfold(x, k, padding=p, stride=s)  # (cb, Cin*k*k, Ho*Wo), rows ordered (c, ky, kx) like w.reshape
        y[i:i + cb] = (wm @ cols).view(-1, cout, Ho, Wo)
        A[i:i + cb] = (wa @ cols.abs()).view(-1, cout, Ho, Wo)
        del x, cols
    if b is not None:
        bb = b.to(device=dev, dtype=torch.float64).view(1, -1, 1, 1)
        y += bb
        A += bb.abs()
    if addz is not None:
        z, za = resize_addz(addz.to(device=dev, dtype=torch.float64), Ho, Wo)
        y += z
        A += za
    y = _act(y, act) * out_scale
    Y = y.abs()
    if res is not None:
        r = res.to(device=dev, dtype=torch.float64)
        y += r
        Y += r.abs()
    return y, A, Y


def nterms(cin, k, addz=False):
    """accumulated terms of one output: the taps, the bias, the four bilinear addz taps."""
    return cin * k * k + 1 + (4 if addz else 0)


def bound(y, A, Y, K, out_scale=1.0, f16_out=True):
    """|got - y| <= 1.1 K 2^-23 |out_scale| A + 2^-22 Y + ulp16(y): fp32 accumulation of K terms in any order (slope of
    SiLU <= 1.1), the fp32 activation / scale / residual add, one f16 output rounding (A, Y: see conv_ref)."""
    b = (1.1 * K * 2.0 ** -23 * abs(out_scale)) * A + 2.0 ** -22 * Y
    return b + ulp16(y) if f16_out else b


def propagate(err, w2, k, s, p, slope=1.1):
    """Bound of the error a second conv stage inherits from an error map `err` of its input: slope * sum |w2| err."""
    e, _, _ = conv_ref([err], w2.abs(), None, k, s, p)
    return slope * e


def mid_error(b1, mid):
    """Error of the f16 intermediate a fused kernel keeps against the f16-rounded fp64 intermediate: the first stage's
    bound plus one f16 ulp (an fp32 value within b1 of the reference may round to the neighbouring f16)."""
    return b1 + ulp16(mid)


def report(case, label, got, y, bnd=None, mean_ulp_max=0.5):
    """Per-element bound + mean-ulp check of a kernel output `got` (any float dtype) against the fp64 reference `y`.
    Prints the case, the kernel label, max err/bound and mean |err|/ulp16(y); returns (max err/bound, mean ulp)."""
    g = got.to(device=y.device, dtype=torch.float64)
    err = (g - y).abs()
    assert torch.isfinite(g).all(), f"{case} [{label}]: non-finite output"
    mu = float((err / ulp16(y)).mean())
    rb = float((err / bnd).max()) if bnd is not None else float("nan")
    print(f"[fp64] {case} [{label}] max err/bound {rb:.3f}  mean ulp {mu:.3f}  max |y| {float(y.abs().max()):.3g}")
    if bnd is not None:
        bad = err > bnd
        if bool(bad.any()):
            i = int(torch.nonzero(bad.flatten())[0])
            raise AssertionError(f"{case} [{label}]: {int(bad.sum())} elements exceed the fp64 bound (max err/bound {rb:.3f}); first at flat index {i}: "
                                 f"got {float(g.flatten()[i])} want {float(y.flatten()[i])} bound {float(bnd.flatten()[i]):.3g}")
    assert mu <= mean_ulp_max, f"{case} [{label}]: mean error {mu:.3f} ulp16 > {mean_ulp_max}"
    return rb, mu


def assert_exact(case, label, got, y):
    """got (f16 / f32 kernel output) must equal the fp64 reference rounded to its dtype, bit for bit."""
    want = y.to(got.dtype)
    assert torch.equal(want.double(), y), f"{case}: the fp64 reference is not exactly representable in {got.dtype} (max |y| {float(y.abs().max())})"
    g = got.to(y.device)
    if not torch.equal(g, want):
        d = (g.double() - want.double()).abs()
        n = int((d > 0).sum())
        i = int(torch.argmax(d.flatten()))
        idx = [int(v) for v in torch.unravel_index(torch.tensor(i), tuple(d.shape))]
        raise AssertionError(f"{case} [{label}]: {n} of {d.numel()} elements differ from the exact fp64 result; worst at (b,c,y,x)={idx}: "
                             f"got {float(g.flatten()[i])} want {float(want.flatten()[i])}")
    print(f"[exact] {case} [{label}] bit-exact, {y.numel()} elements")


# ---- exact-arithmetic data recipe: every partial sum is exact in fp32, outputs < 512 are exact in f16
def ex_input(shape, gen, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def ex_weight(shape, gen):
    return torch.randint(-4, 5, shape, generator=gen).double() / 4  # multiples of 1/4 in [-1, 1]


def ex_bias(n, gen):
    return torch.randint(-8, 9, (n,), generator=gen).float() / 4


def ex_sparse_weight(shape, gen, density=0.25):
    """multiples of 1/4 with most taps zero: keeps |y| < 512 at K in the thousands (inputs |x| <= 2)."""
    w = ex_weight(shape, gen)
    return w * (torch.rand(shape, generator=gen) < density)


def safe_density(K, cap=400.0):
    """density of ex_sparse_weight that keeps the expected max |y| of K taps well below 512."""
    return min(1.0, cap / (2.0 * K)) if K > 0 else 1.0


def stage(w, b=None, k=1, s=1, p=0, act=ACT_NONE, dw=False, addz=None, out_scale=1.0, res=None, K=None):
    """One conv of a fused chain for check_chain: w as the kernel holds it (f16-rounded in f16 mode), b fp32; dw = depthwise
    (w is (C, 1, k, k)); addz / out_scale / res as in conv_ref.  K: accumulated terms of one output where the default (the taps,
    the bias, the addz taps) overstates them (a stage without a bias)."""
    return dict(w=w, b=b, k=k, s=s, p=p, act=act, dw=dw, addz=addz, out_scale=out_scale, res=res, K=K)


def _dense(w):
    c, k = w.shape[0], w.shape[-1]
    d = torch.zeros((c, c, k, k), dtype=torch.float64, device=w.device)
    d[torch.arange(c), torch.arange(c)] = w[:, 0].double()
    return d


def chain_ref(srcs, stages, up=None, f16_points=True, on_stage=None):
    """(y, bound) of the last of `stages` run back to back on `srcs`, every intermediate rounded to f16 where a fused kernel rounds
    it: the bound of a stage is its own bound (`bound`) plus the error its input inherits (`propagate` of `mid_error` of the stage
    before).  on_stage(i, y, bound) is called for every stage.  f16_points=False: nothing is rounded (the plain fp64 composition; the
    bound returned then only describes a kernel that keeps fp32 intermediates)."""
    x, err = list(srcs), None
    for i, st in enumerate(stages):
        w = _dense(st["w"]) if st["dw"] else st["w"]
        y, A, Y = conv_ref(x, w, st["b"], st["k"], st["s"], st["p"], st["act"], up=up if i == 0 else None, addz=st["addz"],
                           out_scale=st["out_scale"], res=st["res"])
        K = st.get("K") or (1 if st["dw"] else w.shape[1]) * st["k"] ** 2 + 1 + (4 if st["addz"] is not None else 0)
        bnd = bound(y, A, Y, K, st["out_scale"])
        if err is not None:
            bnd = bnd + propagate(err, w, st["k"], st["s"], st["p"]) * abs(st["out_scale"])
        if on_stage is not None:
            on_stage(i, y, bnd)
        if i == len(stages) - 1:
            return y, bnd
        mid = y.to(torch.float16).double() if f16_points else y
        err = mid_error(bnd, mid) if f16_points else bnd
        x = [mid]


def check_chain(case, label, got, srcs, stages, up=None, got_mid=None):
    """A fused kernel that runs `stages` back to back and keeps every intermediate as f16: the fp64 reference rounds each
    intermediate to f16 where the kernel rounds it; the bound of a stage is its own bound (`bound`) plus the error its input
    inherits (`propagate` of `mid_error` of the stage before).  got_mid: optional {stage index: kernel output of that stage}
    (fused kernels that also write an intermediate).  Returns (max err/bound, mean ulp) of the final output."""
    def mids(i, y, bnd):
        if got_mid is not None and i in got_mid and i < len(stages) - 1:
            report(f"{case} stage {i}", label, got_mid[i], y, bnd)

    y, bnd = chain_ref(srcs, stages, up=up, on_stage=mids)
    return report(case, label, got, y, bnd)


# ---- graph form: stages name their sources / res / addz by key (block programs: nn/_block.py, csrc/block.hip)
def gnode(out, srcs, w=None, b=None, k=1, s=1, p=None, act=ACT_NONE, dw=False, addz=None, out_scale=1.0, res=None, K=None, op="conv",
          into=None, ngroup=1, taps=None):
    """One stage of graph_ref.  out: key of the result.  srcs: 1-2 source specs, each a key or (key, lo, hi) = a channel slice.
    op "conv": w / b / k / s / p / act / dw / addz / out_scale / res / K as in `stage`, res and addz being source specs; with
    ngroup > 1 the single source holds ngroup channel groups side by side, w and b are lists of weight sets (group g takes set
    min(g, len - 1)), and res / addz / the result hold ngroup * Cout channels.  op "dwt": taps (4, 2, 2) as the kernel holds them,
    stride 2, result [LL | LH | HL | HH].  op "pool": result [y1 | y2 | y3], y_i = max_pool2d(5, 1, 2) applied i times.
    into = (key, lo): the (f16-rounded) result also replaces channels [lo, lo + C) of tensor `key` (a stage that writes in place)."""
    return dict(out=out, srcs=list(srcs), w=w, b=b, k=k, s=s, p=k // 2 if p is None else p, act=act, dw=dw, addz=addz, out_scale=out_scale,
                res=res, K=K, op=op, into=into, ngroup=ngroup, taps=taps)


def _gget(env, spec):
    if spec is None:
        return None, None
    key, lo, hi = (spec, None, None) if isinstance(spec, str) else spec
    v, e = env[key]
    if lo is None:
        return v, e
    return v[:, lo:hi], (e[:, lo:hi] if e is not None else None)


def _gcat_err(vals, errs):
    if all(e is None for e in errs):
        return None
    return torch.cat([e if e is not None else torch.zeros_like(v) for v, e in zip(vals, errs)], 1)


def _gconv(nd, xs, es, w, b, z, ze, r, re):
    w = _dense(w) if nd["dw"] else w
    k, s, p = nd["k"], nd["s"], nd["p"]
    y, A, Y = conv_ref(xs, w, b, k, s, p, nd["act"], addz=z, out_scale=nd["out_scale"], res=r)
    K = nd["K"] or (1 if nd["dw"] else w.shape[1]) * k ** 2 + 1 + (4 if z is not None else 0)
    bnd = bound(y, A, Y, K, nd["out_scale"])
    err = _gcat_err(xs, es)
    if err is not None:
        bnd = bnd + propagate(err, w, k, s, p) * abs(nd["out_scale"])
    if ze is not None:  # an erroneous addz map passes the bilinear taps (convex weights) and the activation
        bnd = bnd + 1.1 * resize_addz(ze, y.shape[2], y.shape[3])[0] * abs(nd["out_scale"])
    if re is not None:
        bnd = bnd + re
    return y, bnd


def graph_ref(inputs, nodes, f16_points=True, on_node=None, device=None):
    """fp64 reference of a DAG of stages (`gnode`).  inputs {key: tensor} carry no error; a stage's result is kept, for the stages
    that read it, rounded to f16 where the kernels round it, with error mid_error(bound of that stage).  A stage's bound is
    bound(...) plus `propagate` over each erroneous source plus the error of an erroneous res (and addz); two sources concatenate
    along channels before conv_ref, as the kernels do.  Returns {out key: (y, bound)} with y unrounded; on_node(nd, y, bound) is
    called per stage.  f16_points=False: nothing is rounded (plain fp64 composition)."""
    dev = device or next(iter(inputs.values())).device
    env = {k: (v.to(device=dev, dtype=torch.float64), None) for k, v in inputs.items()}
    res = {}
    for nd in nodes:
        got = [_gget(env, sp) for sp in nd["srcs"]]
        xs, es = [g[0] for g in got], [g[1] for g in got]
        if nd["op"] == "conv":
            z, ze = _gget(env, nd["addz"])
            r, re = _gget(env, nd["res"])
            ng = nd["ngroup"]
            if ng == 1:
                y, bnd = _gconv(nd, xs, es, nd["w"], nd["b"], z, ze, r, re)
            else:
                assert len(xs) == 1 and xs[0].shape[1] % ng == 0
                ci, ys, bs = xs[0].shape[1] // ng, [], []
                co = nd["w"][0].shape[0]

                def grp(t, g, c):
                    return t[:, g * c:(g + 1) * c] if t is not None else None
                for g in range(ng):
                    q = min(g, len(nd["w"]) - 1)
                    yg, bg = _gconv(nd, [grp(xs[0], g, ci)], [grp(es[0], g, ci)], nd["w"][q], nd["b"][q] if nd["b"] is not None else None,
                                    grp(z, g, co), grp(ze, g, co), grp(r, g, co), grp(re, g, co))
                    ys.append(yg)
                    bs.append(bg)
                y, bnd = torch.cat(ys, 1), torch.cat(bs, 1)
        elif nd["op"] == "dwt":
            c = xs[0].shape[1]
            taps = nd["taps"].to(device=dev, dtype=torch.float64)
            ys, bs = [], []
            for band in range(4):
                wd = _dense(taps[band].expand(c, 1, 2, 2))
                yb, A, Y = conv_ref(xs, wd, None, 2, 2, 0)
                bb = bound(yb, A, Y, 4)
                if es[0] is not None:
                    bb = bb + propagate(es[0], wd, 2, 2, 0, slope=1.0)
                ys.append(yb)
                bs.append(bb)
            y, bnd = torch.cat(ys, 1), torch.cat(bs, 1)
        elif nd["op"] == "pool":  # max of f16 values: exact; an input error passes through the max unchanged
            ys, bs, v, e = [], [], xs[0], es[0]
            for _ in range(3):
                v = F.max_pool2d(v, 5, 1, 2)
                e = F.max_pool2d(e, 5, 1, 2) if e is not None else None
                ys.append(v)
                bs.append(e if e is not None else torch.zeros_like(v))
            y, bnd = torch.cat(ys, 1), torch.cat(bs, 1)
        else:
            raise ValueError(nd["op"])
        if on_node is not None:
            on_node(nd, y, bnd)
        res[nd["out"]] = (y, bnd)
        if nd["op"] == "pool":
            mid, err = y, (bnd if es[0] is not None else None)
        else:
            mid = y.to(torch.float16).double() if f16_points else y
            err = mid_error(bnd, mid) if f16_points else bnd
        env[nd["out"]] = (mid, err)
        if nd["into"] is not None:
            key, lo = nd["into"]
            v, e = env[key]
            v, e = v.clone(), (e.clone() if e is not None else torch.zeros_like(v))
            v[:, lo:lo + mid.shape[1]] = mid
            e[:, lo:lo + mid.shape[1]] = err if err is not None else 0
            env[key] = (v, e)
    return res


def check_graph(case, label, got, inputs, nodes, mean_ulp_max=0.5):
    """got {out key: kernel output}: each against graph_ref's y and bound (`report`).  Returns {key: (max err/bound, mean ulp)}."""
    ref = graph_ref(inputs, nodes)
    return {k: report(f"{case} {k}", label, g, ref[k][0], ref[k][1], mean_ulp_max) for k, g in got.items()}
