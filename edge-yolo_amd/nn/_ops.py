"""Tensor-level wrappers over the C ABI: take logical-NCHW torch tensors (NHWC memory), hand plain pointers /
strides to libedgeyolo_hip.so on the current HIP stream.  No arithmetic happens in Python or in torch here."""
import collections
import ctypes

import torch

from .. import _lib as L

TRACE = None  # set by edge-yolo_amd/profiling.py: per-launch HIP-event timing + algorithmic bytes/FLOPs
RECORD = None  # set by nn/_block.py while a block program is being recorded: wrappers append a stage instead of launching


def _no_block(what):
    if RECORD is not None:
        from ._block import BlockUnsupported
        raise BlockUnsupported(what)


class _NoTrace:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NT = _NoTrace()


def _tr(kernel, nbytes, flops=0, note="", kernels=1):
    return TRACE.launch(kernel, nbytes, flops, note, kernels) if TRACE is not None else _NT


def _nb(*tensors):
    """algorithmic bytes: every listed tensor view touched exactly once."""
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


def _dev_key(x, tag=""):
    return (tag, x.dtype, x.device)


def _act_code(act):
    from .modules.conv import _act_code as code  # (modules.conv imports this module: resolved at call time)
    return code(act)


def _p(t):
    """Pointer of an optional tensor: None (NULL) when it is absent."""
    return None if t is None else t.data_ptr()


def _pcs(t):
    """(pointer, pixel stride) of an optional NHWC view: (None, 0) when it is absent."""
    return (None, 0) if t is None else (t.data_ptr(), L.cstride(t))


def _carray(ctype, values):
    """ctypes array of `values`; an array handed to C never has zero elements (an empty input gives one zero element)."""
    values = list(values)
    return (ctype * max(len(values), 1))(*values)


def _ia(values):
    return _carray(ctypes.c_int, values)


def _la(values):
    return _carray(ctypes.c_long, values)


def _fa(values):
    return _carray(ctypes.c_float, values)


def _pa(tensors):
    """void* array of the tensors' pointers (NULL for None)."""
    return _carray(ctypes.c_void_p, [_p(t) for t in tensors])


def _aligned16(t, channels=True, width=16):
    """True when the NHWC view `t` starts on a `width`-byte boundary and its pixel stride is a multiple of `width` bytes (what the kernels' vector
    accesses need); channels: and its channel count is a multiple of 8."""
    return not ((channels and t.shape[1] % 8) or (L.cstride(t) * t.element_size()) % width or t.data_ptr() % width)


def _nhwc_view(t, what, shape, dtype, slot=False):
    """`t` must be an NHWC view of exactly `shape` and `dtype`; slot: whose channel window (a multiple of 8 channels) starts on a 16-byte boundary
    with a 16-byte pixel stride."""
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not L.is_nhwc_view(t):
        raise ValueError(f"{what} must be an NHWC view of shape {tuple(shape)} {dtype}, got {tuple(t.shape)} {t.dtype}")
    if slot and not _aligned16(t):
        raise ValueError(f"{what}: {t.shape[1]} channels at pixel stride {L.cstride(t)}: channel counts, slot offsets and strides must be multiples of 8 elements")
    return t


def _out(what, out, shape, dtype, device, slot=False):
    """The output of the op `what` (names the argument too, "conv2d: out="): a new NHWC tensor when `out` is None, else `out` after _nhwc_view's
    check -- the kernels trust the pointer and the pixel stride they are given, a wrong view would be written past its end."""
    return L.empty_nhwc(*shape, dtype, device) if out is None else _nhwc_view(out, what, shape, dtype, slot)


class _AtLeast(int):
    """An extent of a _dense shape pattern that is a lower bound, not an exact size."""

    def __repr__(self):
        return f">={int(self)}"


_ANY = _AtLeast(0)


def _dense(t, what, dtype, shape, device):
    """`t` (`what` names the op and the argument, "mask_iou: pred") must be a contiguous tensor of `dtype` (or of one of a tuple of dtypes) on
    `device` whose shape matches `shape`: a plain int is an exact extent, _AtLeast(n) a lower bound, _ANY any extent.  device: a torch.device
    without an index takes every device of its type; None takes the tensor wherever it lives (the caller's require_device follows)."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    ok = torch.is_tensor(t) and t.dtype in dtypes and t.dim() == len(shape) and t.is_contiguous() and all(
        g >= w if isinstance(w, _AtLeast) else g == w for g, w in zip(t.shape, shape))
    if ok and device is not None:
        ok = t.device.type == device.type and device.index in (None, t.device.index)
    if not ok:
        given = f"{t.dtype} {tuple(t.shape)}{'' if t.is_contiguous() else ' (not contiguous)'} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what} must be a contiguous {' or '.join(str(d).replace('torch.', '') for d in dtypes)} tensor of shape {tuple(shape)}"
                         f"{'' if device is None else f' on {device}'}, got {given}")
    return t


def _dense_out(what, out, dtype, shape, device, fill=None):
    """The dense output of the op `what` ("scale_masks: out="): `out` after _dense's check, or, when it is None, a new tensor of `shape` (a lower
    bound allocates exactly the bound) holding `fill` everywhere when one is given."""
    if out is not None:
        return _dense(out, what, dtype, shape, device)
    shape = tuple(int(v) for v in shape)
    return torch.empty(shape, dtype=dtype, device=device) if fill is None else torch.full(shape, fill, dtype=dtype, device=device)


def _workspace(what, ws, nbytes, device, align=16):
    """The scratch buffer of the op `what`: a new uint8 buffer of max(nbytes, 16) bytes when `ws` is None, else `ws` after checking that it is a
    contiguous uint8 buffer of at least `nbytes` bytes on `device` that starts on an `align`-byte boundary, as the entry points document."""
    if ws is None:
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    _dense(ws, f"{what}: workspace", torch.uint8, (_AtLeast(nbytes),), device)
    if ws.data_ptr() % align:
        raise ValueError(f"{what}: workspace must start on a {align}-byte boundary")
    return ws


def _pair_offsets(what, pred_off, gt_off, out_off=None):
    """The host lists of an op that writes one [M_b][N_b] matrix per image into a flat buffer: pred_off / gt_off (B+1 entries from 0) group the
    rows by image, out_off[b] is where image b's matrix starts (default: packed one after the other).  -> (pred_off, gt_off, out_off) as int
    lists, the matrices' sizes and the end of the flat buffer (images without a matrix do not count: their out_off is ignored)."""
    pred_off, gt_off = [int(v) for v in pred_off], [int(v) for v in gt_off]
    B = len(pred_off) - 1
    if B < 0 or len(gt_off) != B + 1 or pred_off[0] != 0 or gt_off[0] != 0:
        raise ValueError(f"{what}: pred_off and gt_off must have B+1 entries starting at 0")
    sizes = [(gt_off[b + 1] - gt_off[b]) * (pred_off[b + 1] - pred_off[b]) for b in range(B)]
    if out_off is None:
        out_off = [0] * B
        for b in range(1, B):
            out_off[b] = out_off[b - 1] + sizes[b - 1]
    out_off = [int(v) for v in out_off]
    if len(out_off) != B or any(o < 0 for o, s in zip(out_off, sizes) if s):
        raise ValueError(f"{what}: out_off must have B = {B} entries, none of them negative where the image has a matrix")
    return pred_off, gt_off, out_off, sizes, max([o + s for o, s in zip(out_off, sizes) if s] + [0])


def _nms_out(B, max_det, width, device):
    """The outputs every NMS entry point fills: rows fp32 (B, max_det, width), count int32 (B,), index int32 (B, max_det)."""
    return (torch.empty((B, max_det, width), dtype=torch.float32, device=device), torch.empty((B,), dtype=torch.int32, device=device),
            torch.empty((B, max_det), dtype=torch.int32, device=device))


def _try_launch(rec, what, fn, *args, kernel=None):
    """Call the fused-op entry fn(*args) under the trace record `rec`.  False when it answers EY_EUNSUPPORTED, which the C side returns before
    anything is launched (`rec` is dropped by its __exit__): the caller then composes the op from its parts.  kernel: called after a launch
    under trace() for the name of the kernel that ran."""
    try:
        with rec:
            L.check(fn(*args), what)
            if kernel is not None and rec is not _NT:
                rec.kernel = kernel()
    except NotImplementedError:
        return False
    return True


class VirtualCat:
    """Channel concat of NHWC tensors that is never written: `parts` = [(tensor, up)], `up`=1 meaning "read through a
    nearest x2 upsample".  Produced by Upsample / Concat when the graph knows the consumer is a 1x1 conv (layers
    11-12, 14-15, 18, 21 of the YAMLs); the conv kernel walks the sources directly (K7 folded into K1)."""

    def __init__(self, parts):
        self.parts = parts
        t, u = parts[0]
        self.shape = (t.shape[0], sum(p.shape[1] for p, _ in parts), t.shape[2] << u, t.shape[3] << u)
        self.dtype, self.device = t.dtype, t.device
        self.is_cuda = t.is_cuda

    def dim(self):
        return 4

    def materialize(self):
        B, c, H, W = self.shape
        out = L.empty_nhwc(B, c, H, W, self.dtype, self.device)
        c0 = 0
        for t, u in self.parts:
            copy_slice(L.as_nhwc(t), out[:, c0:c0 + t.shape[1]], up=u)
            c0 += t.shape[1]
        return out


def as_tensor(x):
    return x.materialize() if isinstance(x, VirtualCat) else x


def pack_conv_weight(w_oihw, dtype, device):
    """fp32 OIHW -> packed MFMA layout (host side, ey_conv_pack_weight) -> device."""
    w = w_oihw.detach().float().cpu().contiguous()
    co, ci, k, _ = w.shape
    code = L.dtype_code(dtype)
    nbytes = L.lib().ey_conv_packed_bytes(code, co, ci, k)
    buf = torch.empty(nbytes, dtype=torch.uint8)
    L.check(L.lib().ey_conv_pack_weight(code, co, ci, k, w.data_ptr(), buf.data_ptr(), nbytes), "conv_pack_weight")
    return buf.to(device)


def _conv_pack(mod, x0, cin, k, tag="", folded_fn=None, w_sets=1):
    """(packed MFMA weights, fp32 bias or None, Cout, elements per weight set) of a conv reading `cin` channels of x0's dtype / device, cached on
    `mod` in the slot "igemm" + tag.  folded_fn() -> fp32 (w, b), mod.folded by default; with w_sets > 1 a list of them (group g of a grouped
    conv uses set min(g, w_sets - 1)): packed back to back, biases stacked."""
    def build():
        ws, bs = zip(*([(folded_fn or mod.folded)()] if w_sets == 1 else (folded_fn or mod.folded)()))
        for w in ws:
            if w.shape[1] != cin or w.shape[2] != k or w.shape[0] != ws[0].shape[0]:
                raise ValueError(f"conv: weight {tuple(w.shape)} does not match Cin={cin} k={k}")
        packs = [pack_conv_weight(w, x0.dtype, x0.device) for w in ws]
        bias = None if bs[0] is None else torch.cat([b.to(x0.device).float() for b in bs]).contiguous()
        return torch.cat(packs), bias, ws[0].shape[0], packs[0].numel() // x0.element_size()

    return mod._packed(_dev_key(x0, "igemm" + tag), build)


def _stem_pack(mod, x, folded_fn):
    """fp32 OIHW weights and bias of an image stem on x's device, in the one cache slot every stem kernel reads."""
    def build():
        w, b = folded_fn()
        return w.to(x.device).contiguous(), b.to(x.device).contiguous()

    return mod._packed(("stem", x.device), build)


def _dw_pack(mod, x, folded_fn, c, k, tag):
    """Depthwise weights [k][k][C] in x's dtype and the fp32 bias (const float* in every depthwise entry point) or None, cached on `mod` in
    the slot `tag`.  folded_fn() -> (w (C,1,k,k), b or None)."""
    def build():
        w, b = folded_fn()
        wk = w.view(c, k, k).permute(1, 2, 0).contiguous().to(device=x.device, dtype=x.dtype)
        return wk, (None if b is None else b.to(x.device).float().contiguous())

    return mod._packed(_dev_key(x, tag), build)


def igemm_ok(srcs, k, s, p):
    if k not in (1, 3) or s not in (1, 2) or p != k // 2:
        return False
    for t in srcs:  # (a plain loop: this runs once per conv launch of an eager forward)
        if not _aligned16(t):
            return False
    return True


_CONV_VARIANTS = (  # (lowest ey_conv_last_variant code of the range, kernel name): h, t, u = the code's hundreds, tens and units, ht = h and t together
    (13000, "conv_igemm_kernel<{tn},{ht},{u}>"), (12000, "conv_ws_kernel<{tn},{h},{t},{u}>"), (11000, "conv3_halo_kernel<{tn},{ht},{u}>"),
    (10000, "conv_small_kernel<{tn},{ht},{u}>"), (9000, "conv3p_kernel<{ht}>"), (8000, "conv3s_kernel<{h},{t},{u}>"), (7000, "conv3r_kernel<{ht},{u}>"),
    (6000, "conv3_tile_kernel<{tn},{ht},{u}>"), (5000, "conv_pwr_kernel<{tn},{ht},{u}>"), (4000, "conv_pw_kernel<{tn},{ht}>"),
    (3000, "conv_pwn_kernel<{tn},{ht},{u}>"))


def _conv_variant(lv, tn):
    """Kernel instantiation behind the code ey_conv_last_variant() reports after an ey_conv2d launch; tn: "f16" or "f32"."""
    for floor, name in _CONV_VARIANTS:
        if lv >= floor:
            return name.format(tn=tn, ht=lv % 1000 // 10, h=lv % 1000 // 100, t=lv % 100 // 10, u=lv % 10)
    # every launch path of ey_conv2d reports its instantiation
    raise AssertionError(f"ey_conv2d launched without reporting its kernel (variant {lv})")


def conv2d(mod, srcs, folded_fn, k, s, p, act, out=None, res=None, tag="", up=None, addz=None, out_scale=1.0,
           ngroup=1, src_gstride=0, y_gstride=0, group_C=None, w_sets=1, _build_only=False):
    """y = res + out_scale*act(conv(cat(srcs)) + bias + up2x(addz)).  srcs: list of 1-2 logical-NCHW tensors
    (source i is read through a nearest x2 upsample when up[i]).  With ngroup>1 `srcs[0]`/`out` are the group-0
    slices and *_gstride the element offsets between groups (channel count per group = group_C)."""
    if len(srcs) == 1 and isinstance(srcs[0], VirtualCat):
        vc = srcs[0]
        if k == 1 and len(vc.parts) <= 2 and up is None:
            srcs, up = [t for t, _ in vc.parts], [u for _, u in vc.parts]
        else:
            srcs = [vc.materialize()]
    x0 = srcs[0]
    L.require_device(x0, "conv2d")
    srcs = [L.as_nhwc(t) for t in srcs]
    up = up or [0] * len(srcs)
    B = srcs[0].shape[0]
    H = srcs[0].shape[2] << up[0]
    W = srcs[0].shape[3] << up[0]
    for t, u in zip(srcs, up):
        if (t.shape[0], t.shape[2] << u, t.shape[3] << u) != (B, H, W) or t.dtype != x0.dtype:
            raise ValueError(f"conv2d: sources disagree: {[tuple(t.shape) for t in srcs]} up={up}")
    cin = sum(t.shape[1] for t in srcs)
    if len(srcs) > 2 or not igemm_ok(srcs, k, s, p):
        if _build_only:
            return None
        _no_block("conv shape outside the MFMA kernel")
        if len(srcs) != 1 or up[0] or addz is not None or ngroup != 1 or out_scale != 1.0:
            raise NotImplementedError("this conv shape needs the generic direct kernel, which takes a single plain source")
        return conv2d_direct(mod, srcs[0], folded_fn, k, s, p, 1, act, out=out, res=res, tag=tag)
    dtype, dev = x0.dtype, x0.device
    wp, bias, cout, wset_elems = _conv_pack(mod, x0, cin, k, tag, folded_fn, w_sets)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    # a grouped conv is given the group-0 slice of its output (Cout channels), or allocates every group's channels when the groups share a pixel
    out = _out("conv2d: out=", out, (B, cout * (ngroup if out is None and y_gstride == 0 and ngroup > 1 else 1), Ho, Wo), dtype, dev)
    d = L.ConvDesc()
    d.dtype = L.dtype_code(dtype)
    d.B, d.H, d.W, d.Ho, d.Wo, d.Cout = B, H, W, Ho, Wo, cout
    d.k, d.stride, d.pad, d.act, d.nsrc = k, s, p, act, len(srcs)
    for i, t in enumerate(srcs):
        d.src[i] = t.data_ptr()
        d.src_C[i] = group_C if (group_C and i == 0) else t.shape[1]
        d.src_cstride[i] = L.cstride(t)
        d.src_up[i] = up[i]
    d.w = wp.data_ptr()
    d.bias = _p(bias)
    d.y, d.y_cstride = out.data_ptr(), L.cstride(out)
    if res is not None:
        res = L.as_nhwc(res)
        if tuple(res.shape) != (B, cout, Ho, Wo) or res.dtype != dtype:
            raise ValueError("conv2d: residual shape/dtype mismatch")
        d.res, d.res_cstride = res.data_ptr(), L.cstride(res)
    d.out_scale = float(out_scale)
    if addz is not None:
        addz = L.as_nhwc(addz)
        if tuple(addz.shape[:2]) != (B, cout) or addz.dtype != dtype:
            raise ValueError("conv2d: addz batch/channel/dtype mismatch")
        d.addz, d.addz_cstride, d.addz_H, d.addz_W = addz.data_ptr(), L.cstride(addz), addz.shape[2], addz.shape[3]
    d.ngroup, d.src_gstride, d.y_gstride = ngroup, src_gstride, y_gstride
    d.w_gstride, d.w_gmax = (wset_elems, w_sets - 1) if w_sets > 1 else (0, 0)
    if _build_only:  # (descriptor, output, tensors the descriptor points into)
        return d, out, (srcs, wp, bias, res, addz)
    if RECORD is not None:
        RECORD.conv(d, srcs, up, out, res, addz, wp, bias, 2.0 * ngroup * B * Ho * Wo * cout * cin * k * k, w_sets * cout * cin * k * k * x0.element_size())
        return out
    if TRACE is not None:
        M = B * Ho * Wo
        es = x0.element_size()
        nbytes = ngroup * (_nb(*srcs) + M * cout * es * (2 if res is not None else 1) + _nb(addz)) + cout * cin * k * k * es
        rec = _tr("conv", nbytes, 2.0 * ngroup * M * cout * cin * k * k,
                  note=f"{cin}->{cout} k{k}s{s} {H}x{W} g{ngroup}{' +res' if res is not None else ''}{' +addz' if addz is not None else ''}{' 2src' if len(srcs) > 1 else ''}")
        with rec:
            L.check(L.lib().ey_conv2d(ctypes.byref(d), L.stream()), "ey_conv2d")
            rec.kernel = _conv_variant(L.lib().ey_conv_last_variant(), "f16" if es == 2 else "f32")
        return out
    L.check(L.lib().ey_conv2d(ctypes.byref(d), L.stream()), "ey_conv2d")
    return out


def pw_chain_packed(mod, x, fold1, fold2):
    """Packed weights of a chained 1x1 pair for ey_conv_pw_chain (cached on `mod`): (w1p, b1, w2p, b2, cmid, cout), or False when the
    pair is outside the chained kernels."""
    cin = x.shape[1]

    def build():
        w1, b1 = fold1()
        w2, b2 = fold2()
        cmid, cout = w1.shape[0], w2.shape[0]
        klen = L.lib().ey_conv_chain_klen(cmid)
        if not klen or w1.shape[2] != 1 or w2.shape[2] != 1 or w2.shape[1] != cmid or not ((cmid == 80 and 64 < cout <= 80 and cout % 4 == 0 and 72 <= cin <= 96) or (cmid == 64 and 1 <= cout <= 16 and 40 <= cin <= 64)):
            return False  # cached: this pair runs as two convs
        perm = (ctypes.c_int * klen)()
        L.check(L.lib().ey_conv_chain_kperm(cmid, perm, klen), "ey_conv_chain_kperm")
        idx = torch.tensor(list(perm), dtype=torch.long)
        w2f = w2.detach().float().cpu()
        w2p = torch.zeros((cout, klen, 1, 1))
        w2p[:, idx >= 0] = w2f[:, idx[idx >= 0]]  # second contraction in the order the first GEMM leaves its results in the registers
        dev = x.device
        return (pack_conv_weight(w1, x.dtype, dev), b1.to(dev).float().contiguous() if b1 is not None else None, pack_conv_weight(w2p, x.dtype, dev),
                b2.to(dev).float().contiguous() if b2 is not None else None, cmid, cout)

    return mod._packed(_dev_key(x, "pwchain"), build)


def packed_conv1x1(mod, x, folded_fn):
    """(packed weight, bias, cout, elements) of a plain 1x1 conv reading `x`, in the cache slot ops.conv2d uses for it."""
    return _conv_pack(mod, x, x.shape[1], 1, folded_fn=folded_fn)


def conv_pw_chain(mod, x, fold1, act1, fold2, act2, out):
    """y = act2(W2 . act1(W1 . x + b1) + b2) in ONE kernel (two chained 1x1 convs, registers only).  Returns None when the shape is
    outside the fused kernel (the caller then runs the two convs)."""
    L.require_device(x, "conv_pw_chain")
    if RECORD is not None:
        return None  # (block programs run the two convs as two stages)
    x = L.as_nhwc(x)
    B, cin, H, W = x.shape
    if x.dtype != torch.float16 or not _aligned16(x):
        return None

    packed = pw_chain_packed(mod, x, fold1, fold2)
    if packed is False:
        return None
    w1p, b1, w2p, b2, cmid, cout = packed
    out = _out("conv_pw_chain: out=", out, (B, cout, H, W), x.dtype, x.device)
    M = B * H * W
    with _tr("conv_pw2_kernel", _nb(x, out) + (cmid * cin + cout * cmid) * 2, 2.0 * M * (cmid * cin + cout * cmid), note=f"{cin}->{cmid}->{cout} {H}x{W}"):
        L.check(L.lib().ey_conv_pw_chain(L.dtype_code(x.dtype), B, H, W, cin, cmid, cout, x.data_ptr(), L.cstride(x), w1p.data_ptr(), _p(b1), act1, w2p.data_ptr(),
                                         _p(b2), act2, out.data_ptr(), L.cstride(out), L.stream()), "ey_conv_pw_chain")
    return out


def conv_pw_pair(a, b):
    """Two chained 1x1 convs as one launch where the shapes allow (ey_conv_pw_pair): `a` / `b` = dict(mod=, folded_fn=, act=, tag=[, srcs=, out=,
    res=, addz=, out_scale=]); b reads a's output.  Returns (y_a, y_b); y_b is None when only the first conv was run (caller runs b itself)."""
    first = dict(mod=a["mod"], srcs=a["srcs"], folded_fn=a["folded_fn"], k=1, s=1, p=0, act=a["act"], out=a.get("out"), res=a.get("res"), addz=a.get("addz"),
                 out_scale=a.get("out_scale", 1.0), tag=a.get("tag", ""))
    x = a["srcs"][0]
    if RECORD is None and len(a["srcs"]) == 1 and torch.is_tensor(x) and x.dtype == torch.float16 and x.is_cuda:
        b1 = conv2d(_build_only=True, **first)
        if b1 is not None:
            d1, y1, keep1 = b1
            b2 = conv2d(b["mod"], [y1], b["folded_fn"], 1, 1, 0, b["act"], out=b.get("out"), tag=b.get("tag", ""), _build_only=True)
            if b2 is not None:
                d2, y2, keep2 = b2
                B, cmid, H, W = y1.shape
                rec = _tr(f"conv_pwc_kernel<f16,{cmid // 16}>", _nb(x, y1, y2, a.get("res"), a.get("addz")), 2.0 * B * H * W * cmid * (x.shape[1] + y2.shape[1]),
                          note=f"{x.shape[1]}->{cmid}->{y2.shape[1]} k1 {H}x{W}")
                if _try_launch(rec, "ey_conv_pw_pair", L.lib().ey_conv_pw_pair, ctypes.byref(d1), ctypes.byref(d2), L.stream()):
                    return y1, y2
    return conv2d(**first), None


def conv2d_direct(mod, x, folded_fn, k, s, p, g, act, out=None, res=None, tag=""):
    L.require_device(x, "conv2d_direct")
    _no_block("direct conv")
    if res is not None:
        raise NotImplementedError("residual add is only fused into the MFMA conv")
    x = L.as_nhwc(x)
    B, cin, H, W = x.shape

    def build():
        w, b = folded_fn()
        return w.to(x.device).contiguous(), (b.to(x.device).contiguous() if b is not None else None)

    w, bias = mod._packed(_dev_key(x, "direct" + tag), build)
    cout = w.shape[0]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    out = _out("conv2d_direct: out=", out, (B, cout, Ho, Wo), x.dtype, x.device)
    d = L.ConvDirectDesc()
    d.dtype = L.dtype_code(x.dtype)
    d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = B, H, W, cin, Ho, Wo, cout
    d.k, d.stride, d.pad, d.groups, d.act = k, s, p, g, act
    d.x, d.x_cstride = x.data_ptr(), L.cstride(x)
    d.w_oihw = w.data_ptr()
    d.bias = _p(bias)
    d.y, d.y_cstride = out.data_ptr(), L.cstride(out)
    with _tr("conv_direct_kernel", _nb(x, out), 2.0 * B * Ho * Wo * cout * (cin // g) * k * k):
        L.check(L.lib().ey_conv2d_direct(ctypes.byref(d), L.stream()), "ey_conv2d_direct")
    return out


def stem_conv(mod, x, folded_fn, act, out_dtype, out=None):
    """3x3/s2 conv straight from the NCHW-contiguous image (layer 0)."""
    L.require_device(x, "stem_conv")
    _no_block("stem conv")
    B, cin, H, W = x.shape
    w, bias = _stem_pack(mod, x, folded_fn)
    cout = w.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = _out("stem_conv: out=", out, (B, cout, Ho, Wo), out_dtype, x.device)
    with _tr("stem_kernel", _nb(x, out), 2.0 * B * Ho * Wo * cout * cin * 9):
        L.check(L.lib().ey_stem_conv(L.dtype_code(x.dtype), L.dtype_code(out_dtype), B, cin, H, W, cout, act, x.data_ptr(), w.data_ptr(),
                                     bias.data_ptr(), out.data_ptr(), L.cstride(out), L.stream()), "ey_stem_conv")
    return out


STEM_KS = {(6, 2, 2): "stem6", (3, 1, 1): "stem3s1", (7, 2, 3): "stem7"}  # (k, s, p) of ey_stem_conv_ks -> trace label stem


def stem_conv_ks(mod, x, folded_fn, k, s, p, act, out_dtype, out=None):
    """The image stems that are not 3x3 stride 2, straight from the NCHW-contiguous image (ey_stem_conv_ks): (k, s, p) = (6, 2, 2) of YOLOv5,
    (3, 1, 1) of YOLOv3 and (7, 2, 3) of the ResNet stem.  out= may be a channel slot of a wider NHWC buffer."""
    L.require_device(x, "stem_conv_ks")
    _no_block("stem conv")
    B, cin, H, W = x.shape
    w, bias = _stem_pack(mod, x, folded_fn)
    cout = w.shape[0]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    if Ho < 1 or Wo < 1:
        raise ValueError(f"stem_conv_ks: a {H}x{W} image has no {k}x{k} window at padding {p}")
    out = _out("stem_conv_ks: out=", out, (B, cout, Ho, Wo), out_dtype, x.device)
    stem = STEM_KS.get((k, s, p), f"stem_k{k}s{s}p{p}")
    rec = _tr(stem + "_kernel", _nb(x, out), 2.0 * B * Ho * Wo * cout * cin * k * k, note=f"{cin}->{cout} k{k}s{s} {H}x{W}")
    with rec:
        L.check(L.lib().ey_stem_conv_ks(L.dtype_code(x.dtype), L.dtype_code(out_dtype), B, cin, H, W, cout, k, s, p, act, x.data_ptr(), w.data_ptr(),
                                        bias.data_ptr(), out.data_ptr(), L.cstride(out), L.stream()), "ey_stem_conv_ks")
        if rec is not _NT and L.lib().ey_stem_conv_ks_last_variant() == 1:
            rec.kernel = stem + "_mfma_kernel"
    return out


def maxpool2d(x, k, s, pad=(0, 0, 0, 0), out=None):
    """nn.MaxPool2d(k, s) behind nn.ZeroPad2d(pad), pad = (left, right, top, bottom) (ey_maxpool2d): the padded cells are ZEROS that take part in
    the maximum.  k = 2 with s = 1 or 2; k = 1, s = 1 is the zero-padded copy.  x and out= may be channel slots of wider NHWC buffers."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "maxpool2d")
    _no_block("max pool")
    B, c, H, W = x.shape
    pl, pr, pt, pb = (int(v) for v in pad)
    if (k, s) not in ((2, 1), (2, 2), (1, 1)):
        raise NotImplementedError(f"maxpool2d: k={k} stride={s}: a 2x2 window with stride 1 or 2 is built (and k = 1, the zero-padded copy)")
    if min(pl, pr, pt, pb) < 0:
        raise NotImplementedError(f"maxpool2d: negative padding {tuple(pad)} (cropping) is not built")
    if c % 8:
        raise NotImplementedError(f"maxpool2d: C={c} must be a multiple of 8")
    Ho, Wo = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
    if Ho < 1 or Wo < 1:
        raise ValueError(f"maxpool2d: a {H}x{W} map padded by {tuple(pad)} has no {k}x{k} window")
    _nhwc_view(x, "maxpool2d: x", x.shape, x.dtype, slot=True)
    out = _out("maxpool2d: out=", out, (B, c, Ho, Wo), x.dtype, x.device, slot=True)
    with _tr("maxpool_kernel" if k > 1 else "zeropad_kernel", _nb(x, out), float(k * k * out.numel()), note=f"C{c} k{k}s{s} pad{(pl, pr, pt, pb)} {H}x{W}"):
        L.check(L.lib().ey_maxpool2d(L.dtype_code(x.dtype), B, H, W, c, k, s, pl, pr, pt, pb, x.data_ptr(), L.cstride(x), out.data_ptr(), L.cstride(out),
                                     L.stream()), "ey_maxpool2d")
    return out


def maxpool3x3s2(x, out=None):
    """nn.MaxPool2d(3, 2, 1) of the ResNet stem (ey_maxpool3x3s2): torch's own padding, the cells outside the map are left out of the maximum.
    Reached from ResNetLayer only; maxpool2d (explicit zero padding that takes part) keeps refusing a 3x3 window.  x and out= may be channel
    slots of wider NHWC buffers."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "maxpool3x3s2")
    _no_block("max pool")
    B, c, H, W = x.shape
    if c % 8:
        raise NotImplementedError(f"maxpool3x3s2: C={c} must be a multiple of 8")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _nhwc_view(x, "maxpool3x3s2: x", x.shape, x.dtype, slot=True)
    out = _out("maxpool3x3s2: out=", out, (B, c, Ho, Wo), x.dtype, x.device, slot=True)
    with _tr("maxpool3x3s2_kernel", _nb(x, out), float(9 * out.numel()), note=f"C{c} {H}x{W}"):
        L.check(L.lib().ey_maxpool3x3s2(L.dtype_code(x.dtype), B, H, W, c, x.data_ptr(), L.cstride(x), out.data_ptr(), L.cstride(out), L.stream()), "ey_maxpool3x3s2")
    return out


def resnet_stem(mod, x, folded_fn, act, out=None):
    """Layer 0 of a ResNet as ONE launch (ey_resnet_stem): Conv 7x7 / 2 / 3 + activation from the NCHW-contiguous image and MaxPool 3x3 / 2 / 1; the
    half-resolution map stays in LDS.  Bit-identical to stem_conv_ks(7, 2, 3) + maxpool3x3s2.  Returns None where the kernel does not take the
    shape (other than 64 output channels, more than 4 input channels): the caller then makes the two launches."""
    L.require_device(x, "resnet_stem")
    _no_block("stem conv")
    B, cin, H, W = x.shape
    w, bias = _stem_pack(mod, x, folded_fn)
    cout = w.shape[0]
    if cout != 64 or cin > 4 or tuple(w.shape[2:]) != (7, 7) or x.dtype not in (torch.float16, torch.float32):
        return None
    Hp, Wp = ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1
    out = _out("resnet_stem: out=", out, (B, cout, Hp, Wp), x.dtype, x.device, slot=True)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rec = _tr("resnet_stem_kernel", _nb(x, out), 2.0 * B * Ho * Wo * cout * cin * 49, note=f"{cin}->{cout} {H}x{W}")
    with rec:
        L.check(L.lib().ey_resnet_stem(L.dtype_code(x.dtype), L.dtype_code(x.dtype), B, cin, H, W, cout, act, x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                       L.cstride(out), L.stream()), "ey_resnet_stem")
        if rec is not _NT and L.lib().ey_resnet_stem_last_variant() == 1:
            rec.kernel = "resnet_stem_mfma_kernel"
    return out


def resnet_tail(mod, t, x, folded_fn, stride, identity, out=None, tag=""):
    """The closing 1x1 of a ResNet bottleneck block as ONE launch (ey_resnet_tail, f16): relu(W [t ; x at pixel stride s] + b) for a projection
    block -- folded_fn() gives ([W3 | Ws] concatenated along K as (4 C2, C2 + C1, 1, 1), b3 + bs) --, relu(W3 t + b3 + x) for an identity block
    (x is the residual, added in fp32 before the ReLU).  Returns None where the kernel does not take the shape (fp32, widths outside its list,
    misaligned views): the caller then takes the composed form."""
    t, x = L.as_nhwc(as_tensor(t)), L.as_nhwc(as_tensor(x))
    L.require_device(t, "resnet_tail")
    _no_block("resnet_tail")
    B, C2, Ho, Wo = t.shape
    _, cx, H, W = x.shape
    C1 = 0 if identity else cx
    if (t.dtype != torch.float16 or x.dtype != torch.float16 or C2 not in (64, 128, 256, 512) or C1 % 32 or C1 > 2048 or stride not in (1, 2) or (identity and (stride != 1 or cx != 4 * C2))
            or x.shape[0] != B or ((H - 1) // stride + 1, (W - 1) // stride + 1) != (Ho, Wo)):
        return None
    if not (_aligned16(t, channels=False) and _aligned16(x, channels=False)):
        return None

    def build():
        w, b = folded_fn()
        return w.reshape(w.shape[0], -1).to(device=t.device, dtype=torch.float16).contiguous(), b.to(device=t.device, dtype=torch.float32).contiguous()

    w, bias = mod._packed(_dev_key(t, "rtail" + tag), build)
    if tuple(w.shape) != (4 * C2, C2 + C1):
        raise ValueError(f"resnet_tail: weight {tuple(w.shape)} does not match (4 C2, C2 + C1) = {(4 * C2, C2 + C1)}")
    out = _out("resnet_tail: out=", out, (B, 4 * C2, Ho, Wo), t.dtype, t.device, slot=True)
    M = B * Ho * Wo
    nbytes = 2 * (M * (C2 + C1 + 4 * C2 * (2 if identity else 1)) + w.numel())
    with _tr("resnet_tail_kernel", nbytes, 2.0 * M * 4 * C2 * (C2 + C1), note=f"{C2}+{C1}->{4 * C2} s{stride} {Ho}x{Wo}{' +res' if identity else ''}"):
        L.check(L.lib().ey_resnet_tail(L.dtype_code(t.dtype), B, H, W, stride, C1, C2, t.data_ptr(), L.cstride(t), *_pcs(None if identity else x), w.data_ptr(), bias.data_ptr(),
                                       *_pcs(x if identity else None), out.data_ptr(), L.cstride(out), L.stream()), "ey_resnet_tail")
    return out


def pw_conv3s2(cv2, conv3, srcs, out=None):
    """A block's closing 1x1 Conv over a two-part virtual concat + the stride-2 3x3 Conv that follows it (layers 2 -> 3 of the n-scale
    backbones: DSC3K2_Wavelet.cv2 / C3k2.cv2, reference block.py:357-396,3783-3788, then conv.py:41-59) as one launch; the 64-channel map
    between them stays in LDS.  Bit-identical to the two launches.  Returns None (nothing launched) outside the fused kernel's shapes."""
    if RECORD is not None or len(srcs) != 2 or any(isinstance(t, VirtualCat) for t in srcs):
        return None
    x0 = srcs[0]
    L.require_device(x0, "pw_conv3s2")
    if x0.dtype != torch.float16:
        return None
    srcs = [L.as_nhwc(t) for t in srcs]
    B, _, H, W = srcs[0].shape
    c1, c3 = cv2.conv, conv3.conv
    if (tuple(srcs[1].shape[0:1] + srcs[1].shape[2:]) != (B, H, W) or c1.kernel_size != (1, 1) or c1.stride != (1, 1) or c1.groups != 1 or c1.out_channels != 64
            or c3.kernel_size != (3, 3) or c3.stride != (2, 2) or c3.padding != (1, 1) or c3.dilation != (1, 1) or c3.groups != 1 or c3.in_channels != 64
            or c3.out_channels != 64 or c1.in_channels != srcs[0].shape[1] + srcs[1].shape[1] or any(t.shape[1] > 32 or t.shape[1] % 8 for t in srcs)
            or _act_code(cv2.act) != L.ACT_SILU or _act_code(conv3.act) != L.ACT_SILU
            or not all(_aligned16(t, channels=False) for t in srcs)):
        return None
    w1, b1 = _conv_pack(cv2, x0, c1.in_channels, 1)[:2]
    w2, b2 = _conv_pack(conv3, x0, 64, 3)[:2]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = _out("pw_conv3s2: out=", out, (B, 64, Ho, Wo), x0.dtype, x0.device)
    c0n, c1n = srcs[0].shape[1], srcs[1].shape[1]
    rec = _tr("pw3_kernel", _nb(srcs[0], srcs[1], out), 2.0 * B * (H * W * 64 * (c0n + c1n) + Ho * Wo * 64 * 576), note=f"{c0n}+{c1n}->64 k1 -> 64 k3s2 {H}x{W}")
    if not _try_launch(rec, "ey_conv_pw_conv3s2", L.lib().ey_conv_pw_conv3s2, L.dtype_code(x0.dtype), B, H, W, srcs[0].data_ptr(), c0n, L.cstride(srcs[0]),
                       srcs[1].data_ptr(), c1n, L.cstride(srcs[1]), 64, w1.data_ptr(), b1.data_ptr(), L.ACT_SILU, 64, w2.data_ptr(), b2.data_ptr(), L.ACT_SILU,
                       out.data_ptr(), L.cstride(out), L.stream()):
        return None
    return out


def scdown(cv1, cv2, x, out=None):
    """SCDown (reference block.py:1174-1206) as one launch (ey_scdown): cv1 = pointwise Conv + activation, cv2 = depthwise 3x3 stride-2 Conv; the
    full-resolution map between them stays in LDS.  Bit-identical to ops.conv2d + ops.dwconv_s2.  x may be a channel slice of a wider NHWC
    buffer, out= a slot of one.  Returns None (nothing launched) outside the fused kernel's shapes: the caller runs the two launches."""
    if RECORD is not None or isinstance(x, VirtualCat) or not torch.is_tensor(x) or x.dim() != 4:
        return None
    L.require_device(x, "scdown")
    if x.dtype != torch.float16:
        return None
    x = L.as_nhwc(x)
    B, c1n, H, W = x.shape
    c1, c2 = cv1.conv, cv2.conv
    k = c2.kernel_size[0]
    cout = c2.out_channels
    if (c1.kernel_size != (1, 1) or c1.stride != (1, 1) or c1.groups != 1 or c1.in_channels != c1n or c1.out_channels != cout or c2.kernel_size != (k, k)
            or k != 3 or c2.stride != (2, 2) or c2.padding != (k // 2, k // 2) or c2.dilation != (1, 1) or not c2.groups == c2.in_channels == cout
            or cout % 64 or not _aligned16(x)):
        return None
    act1, act2 = _act_code(cv1.act), _act_code(cv2.act)
    w1, b1 = _conv_pack(cv1, x, c1n, 1)[:2]
    w2, b2 = _dw_pack(cv2, x, cv2.folded, cout, k, "dw2")  # (the slot ops.dwconv_s2 uses for cv2)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = _out("scdown: out=", out, (B, cout, Ho, Wo), x.dtype, x.device)
    if not _aligned16(out, channels=False):
        return None
    rec = _tr("scdown_kernel", _nb(x, out) + (cout * c1n + 9 * cout) * 2, 2.0 * B * (H * W * cout * c1n + Ho * Wo * cout * k * k), note=f"{c1n}->{cout} k1 -> dw k{k}s2 {H}x{W}")
    if not _try_launch(rec, "ey_scdown", L.lib().ey_scdown, L.dtype_code(x.dtype), B, H, W, c1n, cout, k, x.data_ptr(), L.cstride(x), w1.data_ptr(), _p(b1), act1,
                       w2.data_ptr(), _p(b2), act2, out.data_ptr(), L.cstride(out), L.stream()):
        return None
    return out


def ghost_conv(cv1, cv2, x, out=None, res=None):
    """GhostConv(c1, c2, 1, 1) (reference conv.py:180-193) as one launch (ey_ghost_conv): cv1 = pointwise Conv, cv2 = depthwise 5x5 Conv on
    cv1's output, both with the same activation; out = cat(cv1(x), cv2(cv1(x))) [+ res, an f16 add -- the shortcut of a GhostBottleneck].
    cv1's output stays in LDS.  Where the hidden width is a multiple of 8, bit-identical to ops.conv2d + ops.dwconv (+ the add).  x may be a
    channel slice of a wider NHWC buffer, out= a slot of one, and out= may be res itself.  Returns None (nothing launched) outside the fused
    kernel's shapes: the caller composes."""
    if RECORD is not None or isinstance(x, VirtualCat) or not torch.is_tensor(x) or x.dim() != 4:
        return None
    L.require_device(x, "ghost_conv")
    if x.dtype != torch.float16:
        return None
    x = L.as_nhwc(x)
    B, c1n, H, W = x.shape
    c1, c2 = cv1.conv, cv2.conv
    k = c2.kernel_size[0]
    ch = c1.out_channels
    act = _act_code(cv1.act)
    if (c1.kernel_size != (1, 1) or c1.stride != (1, 1) or c1.groups != 1 or c1.in_channels != c1n or c2.kernel_size != (k, k) or k != 5
            or c2.stride != (1, 1) or c2.padding != (k // 2, k // 2) or c2.dilation != (1, 1) or not c2.groups == c2.in_channels == c2.out_channels == ch
            or ch % 4 or act != _act_code(cv2.act) or not _aligned16(x)):
        return None
    va = 8 if ch % 8 else 16  # (a hidden width of 8 n + 4 channels puts the second half of the output on 8-byte boundaries)
    out = _out("ghost_conv: out=", out, (B, 2 * ch, H, W), x.dtype, x.device)
    if not _aligned16(out, channels=False, width=va):
        return None
    if res is not None:
        res = L.as_nhwc(res)
        if tuple(res.shape) != (B, 2 * ch, H, W) or res.dtype != x.dtype:
            raise ValueError("ghost_conv: residual shape/dtype mismatch")
        if not _aligned16(res, channels=False, width=va):
            return None
    w1, b1 = _conv_pack(cv1, x, c1n, 1)[:2]
    w2, b2 = _dw_pack(cv2, x, cv2.folded, ch, k, "dw")  # (the slot ops.dwconv uses for cv2)
    rec = _tr("ghost_conv_kernel", _nb(x, out, res) + (ch * c1n + k * k * ch) * 2, 2.0 * B * H * W * ch * (c1n + k * k),
              note=f"{c1n}->{ch} k1 -> dw k{k} {H}x{W}{' +res' if res is not None else ''}")
    if not _try_launch(rec, "ey_ghost_conv", L.lib().ey_ghost_conv, L.dtype_code(x.dtype), B, H, W, c1n, ch, k, x.data_ptr(), L.cstride(x), w1.data_ptr(), _p(b1),
                       w2.data_ptr(), _p(b2), act, *_pcs(res), out.data_ptr(), L.cstride(out), L.stream()):
        return None
    return out


def stem_pair(m0, m1, x, out=None):
    """Layers 0 + 1 (Conv 3->16 k3 s2 + Conv 16->32 k3 s2, both BN + SiLU; reference conv.py:41-59) as one launch from the NCHW-contiguous f16
    image: the stem's output -- the largest tensor of the forward, with one consumer -- stays in LDS.  Bit-identical to the two launches.
    Returns None (nothing launched) when the modules / shape are outside the fused kernel."""
    L.require_device(x, "stem_pair")
    if RECORD is not None or x.dtype != torch.float16 or x.dim() != 4 or not x.is_contiguous() or L.is_nhwc_view(x):
        return None
    c0, c1 = m0.conv, m1.conv
    B, cin, H, W = x.shape
    if (cin != 3 or c0.in_channels != 3 or c0.out_channels != 16 or c1.in_channels != 16 or c1.out_channels != 32 or W % 8 or x.data_ptr() % 16
            or any(c.kernel_size != (3, 3) or c.stride != (2, 2) or c.padding != (1, 1) or c.dilation != (1, 1) or c.groups != 1 for c in (c0, c1))):
        return None
    w0, b0 = _stem_pack(m0, x, m0.folded)
    w1, b1 = _conv_pack(m1, x, 16, 3)[:2]
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Ho, Wo = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    out = _out("stem_pair: out=", out, (B, 32, Ho, Wo), x.dtype, x.device)
    rec = _tr("stem_pair_kernel", _nb(x, out), 2.0 * B * (Hs * Ws * 16 * 27 + Ho * Wo * 32 * 144), note=f"3->16->32 {H}x{W}")
    if not _try_launch(rec, "ey_stem_pair", L.lib().ey_stem_pair, B, H, W, x.data_ptr(), w0.data_ptr(), b0.data_ptr(), _act_code(m0.act), 32, w1.data_ptr(), b1.data_ptr(),
                       _act_code(m1.act), out.data_ptr(), L.cstride(out), L.stream()):
        return None
    return out


def dwconv(mod, x, folded_fn, k, act, out=None, tag=""):
    L.require_device(x, "dwconv")
    x = L.as_nhwc(x)
    B, c, H, W = x.shape
    if not _aligned16(x):
        return conv2d_direct(mod, x, folded_fn, k, 1, k // 2, c, act, out=out, tag=tag)
    wk, bias = _dw_pack(mod, x, folded_fn, c, k, "dw" + tag)
    out = _out("dwconv: out=", out, (B, c, H, W), x.dtype, x.device)
    if RECORD is not None:
        RECORD.dw(x, wk, bias, k, act, out)
        return out
    with _tr(f"dwconv_kernel<{k}>", _nb(x, out), 2.0 * x.numel() * k * k, note=f"C{c} {H}x{W}"):
        L.check(L.lib().ey_dwconv(L.dtype_code(x.dtype), B, H, W, c, k, act, x.data_ptr(), L.cstride(x), wk.data_ptr(), _p(bias), out.data_ptr(), L.cstride(out),
                                  L.stream()), "ey_dwconv")
    return out


def _dsconv_pack(mod, x, dw_fn, pw_fn, k):
    """Device operands of one fused DSConv, cached on the module per (dtype, device): depthwise weights [k][k][C], depthwise bias,
    packed pointwise weights (BN folded), bias, Cout, Toeplitz form of the depthwise weights (C 16 / 32) or None."""
    c = x.shape[1]

    def build():
        wd, bd = dw_fn()
        wp, bp = pw_fn()
        # not _dw_pack: the Toeplitz pack below needs the fp32 [k][k][C] weights on the host, and the pack shares one slot with the pointwise half
        wkf = wd.detach().float().view(c, k, k).permute(1, 2, 0).contiguous().cpu()
        wk = wkf.to(device=x.device, dtype=x.dtype)
        tz = None
        if x.dtype == torch.float16 and c in (16, 32) and wp.shape[0] <= 32:  # Toeplitz-MFMA depthwise stage (ey_dsconv_tz)
            nb = L.lib().ey_dsconv_toeplitz_bytes(c, k)
            buf = torch.empty(nb, dtype=torch.uint8)
            w16 = wkf.half().float().contiguous()  # the f16-rounded weights the other kernels use (kept alive across the call)
            L.check(L.lib().ey_dsconv_pack_toeplitz(c, k, w16.data_ptr(), buf.data_ptr(), nb), "ey_dsconv_pack_toeplitz")
            tz = buf.to(x.device)
        return (wk, (bd.to(x.device).float().contiguous() if bd is not None else None), pack_conv_weight(wp, x.dtype, x.device),
                (bp.to(x.device).contiguous() if bp is not None else None), wp.shape[0], tz)

    return mod._packed(_dev_key(x, "dsfused"), build)


def dsb_pair(cv1, cv2, x, add, out=None):
    """DSBottleneck.forward (reference block.py:1496-1503) as one launch: y = [x +] cv2(cv1(x)) for two DSConv modules (k 3 -> 5 / 7, equal
    widths of 32 / 64 channels, f16, small maps).  Bit-identical to the two ey_dsconv launches.  Returns None when the shape is outside
    the fused kernel (nothing launched): the caller then runs the two DSConvs."""
    L.require_device(x, "dsb_pair")
    if RECORD is not None or x.dtype != torch.float16:
        return None
    x = L.as_nhwc(x)
    B, c, H, W = x.shape
    k1, k2 = cv1.dw.kernel_size[0], cv2.dw.kernel_size[0]
    if (c not in (32, 64) or k1 != 3 or k2 not in (5, 7) or cv1.pw.out_channels != c or cv2.pw.out_channels != c or cv2.dw.in_channels != c
            or any(m.dw.stride != (1, 1) or m.dw.dilation != (1, 1) or m.dw.padding != (m.dw.kernel_size[0] // 2,) * 2 or m.dw.bias is not None for m in (cv1, cv2))
            or not _aligned16(x, channels=False)):
        return None
    out = _out("dsb_pair: out=", out, (B, c, H, W), x.dtype, x.device)
    if not _aligned16(out, channels=False):
        return None
    base = x.untyped_storage().data_ptr()
    if out.untyped_storage().data_ptr() == base:
        # same buffer (channel slots of one concat buffer): fine while the channel ranges are disjoint; an overlap (in-place update) would race --
        # a workgroup reads halo rows of x that lie in other workgroups' bands
        cs = L.cstride(x)
        if L.cstride(out) != cs or abs(((x.data_ptr() - base) // 2) % cs - ((out.data_ptr() - base) // 2) % cs) < c:
            return None
    wk1, _, wp1, b1, _, _ = _dsconv_pack(cv1, x, cv1._dw_folded, cv1._pw_folded, k1)
    wk2, _, wp2, b2, _, _ = _dsconv_pack(cv2, x, cv2._dw_folded, cv2._pw_folded, k2)
    rec = _tr(f"dsb_pair_kernel<{k1},{k2}>", _nb(x, out), 2.0 * B * H * W * c * (k1 * k1 + k2 * k2 + 2 * c), note=f"C{c} {H}x{W}{' +res' if add else ''}")
    if not _try_launch(rec, "ey_dsb_pair", L.lib().ey_dsb_pair, L.dtype_code(x.dtype), B, H, W, c, k1, k2, L.ACT_SILU, x.data_ptr(), L.cstride(x), wk1.data_ptr(), wp1.data_ptr(),
                       _p(b1), wk2.data_ptr(), wp2.data_ptr(), _p(b2), 1 if add else 0, out.data_ptr(), L.cstride(out), L.stream()):
        return None
    return out


def dsconv(mod, x, dw_fn, pw_fn, k, act, out=None, res=None, dw_act=0):
    """Fused depthwise->pointwise: y = res + act(pw1x1(dw_act(dw_kxk(x) + dw_bias)) + bias).  Returns None when the shape is
    outside the fused kernel (caller then runs the two-kernel form)."""
    L.require_device(x, "dsconv")
    x = L.as_nhwc(x)
    B, c, H, W = x.shape
    es = x.element_size()
    if c > 256 or not _aligned16(x):
        return None

    wk, dwb, wp, bias, cout, tz = _dsconv_pack(mod, x, dw_fn, pw_fn, k)
    out = _out("dsconv: out=", out, (B, cout, H, W), x.dtype, x.device)
    if res is not None:
        res = L.as_nhwc(res)
    if RECORD is not None:  # two stages: depthwise (rounded to the storage type like the reference's intermediate tensor) -> pointwise 1x1
        t = L.empty_nhwc(B, c, H, W, x.dtype, x.device)
        RECORD.dw(x, wk, dwb, k, dw_act, t)
        d = L.ConvDesc()
        d.dtype, d.B, d.H, d.W, d.Ho, d.Wo, d.Cout = L.dtype_code(x.dtype), B, H, W, H, W, cout
        d.k, d.stride, d.pad, d.act, d.nsrc = 1, 1, 0, act, 1
        d.src_C[0] = c
        d.y_cstride, d.out_scale, d.ngroup = L.cstride(out), 1.0, 1
        RECORD.conv(d, [t], [0], out, res, None, wp, bias, 2.0 * B * H * W * c * cout, cout * c * es)
        return out
    rec = _tr(f"dsconv_kernel<{k}>", _nb(x, out, res), 2.0 * B * H * W * c * (k * k + cout), note=f"C{c}->{cout} {H}x{W}{' +res' if res is not None else ''}")
    head = (L.dtype_code(x.dtype), B, H, W, c, cout, k, act, x.data_ptr(), L.cstride(x), wk.data_ptr())
    tail = (_p(dwb), dw_act, wp.data_ptr(), _p(bias), out.data_ptr(), L.cstride(out), *_pcs(res), L.stream())

    def ran():
        return {2: f"dsconv_strip_kernel<{k}>", 3: f"dsconv_tz_kernel<{k}>"}.get(L.lib().ey_dsconv_last_variant(), rec.kernel)

    if tz is not None:
        ok = _try_launch(rec, "ey_dsconv_tz", L.lib().ey_dsconv_tz, *head, tz.data_ptr(), *tail, kernel=ran)
    else:
        ok = _try_launch(rec, "ey_dsconv", L.lib().ey_dsconv, *head, *tail, kernel=ran)
    return out if ok else None  # (unsupported: the tile does not fit LDS -> the two-kernel form)


def dwt_haar(x, out=None):
    """(B,C,H,W) -> (B,4C,H/2,W/2) with channel blocks LL|LH|HL|HH."""
    L.require_device(x, "dwt_haar")
    x = L.as_nhwc(x)
    B, c, H, W = x.shape
    out = _out("dwt_haar: out=", out, (B, 4 * c, H // 2, W // 2), x.dtype, x.device)
    if RECORD is not None:
        if not _aligned16(x):
            _no_block("dwt alignment")
        RECORD.dwt(x, out)
        return out
    with _tr("dwt_kernel", _nb(x, out), 4.0 * x.numel()):
        L.check(L.lib().ey_dwt_haar(L.dtype_code(x.dtype), B, H, W, c, x.data_ptr(), L.cstride(x), out.data_ptr(), L.cstride(out), L.stream()), "ey_dwt_haar")
    return out


def dwt(x, taps, k, out=None):
    """(B,C,H,W) -> (B,4C,H/2,W/2) with channel blocks LL|LH|HL|HH for a k-tap filter bank (ey_dwt, reflect border).  taps: device
    fp32 (4,k,k), already rounded to x's dtype.  Not a block-program stage: a recorded chain stops here and runs per layer."""
    L.require_device(x, "dwt")
    x = L.as_nhwc(x)
    B, c, H, W = x.shape
    if k // 2 - 1 >= H or k // 2 - 1 >= W:
        raise ValueError(f"dwt: a {k}-tap filter bank reflect-pads by {k // 2 - 1}, which needs a map larger than {H}x{W}")
    _no_block("dwt with a general filter bank")
    out = _out("dwt: out=", out, (B, 4 * c, H // 2, W // 2), x.dtype, x.device)
    with _tr(f"dwt_general_kernel<k{k}>", _nb(x, out), 8.0 * k * k * c * B * (H // 2) * (W // 2)):
        L.check(L.lib().ey_dwt(L.dtype_code(x.dtype), B, H, W, c, k, taps.data_ptr(), x.data_ptr(), L.cstride(x), out.data_ptr(), L.cstride(out),
                               L.stream()), "ey_dwt")
    return out


def wavelet_z(mod, b, sets_fn, z_fn, dwt=None, dw_fn=None):
    """Half-resolution branch of _WaveletEnhancer in ONE kernel (ey_wavelet_z / ey_wavelet_z2): b (B,c,H,W) -> Z (B,c,H/2,W/2).  sets_fn()
    -> ((w_ll3x3, b_ll), (w_h, b_h)) BN-folded fp32 (use_ds: w_h = the pointwise 1x1 as a centre-tap 3x3); z_fn() -> (w_z (c,2c,1,1), None);
    dwt: the _PywtDWT2D (None = Haar); dw_fn (use_ds) -> f_h's depthwise 3x3 weights (c,1,3,3).  Returns None when the shape is outside the
    fused kernel (fp32 mode, c not in {16,32,64,128}, a filter length other than 2/4/6/8, while a block program is recorded): the caller
    runs dwt + the sub-band convs + Z."""
    L.require_device(b, "wavelet_z")
    b = L.as_nhwc(b)
    B, c, H, W = b.shape
    k = 2 if dwt is None or dwt.haar else dwt.k
    if (RECORD is not None or b.dtype != torch.float16 or c not in (16, 32, 64, 128) or k not in (2, 4, 6, 8) or H < 2 or W < 2 or k // 2 - 1 >= min(H, W)
            or not _aligned16(b, channels=False)):
        return None

    def build():
        (wl, bl), (wh, bh) = sets_fn()
        wz, _ = z_fn()
        packs = [pack_conv_weight(w, b.dtype, b.device) for w in (wl, wh)]
        # f_h's depthwise weights [3][3][c]: one member of this op's own pack, not a _dw_pack slot (no bias, no module of their own)
        wdw = dw_fn().float().view(c, 3, 3).permute(1, 2, 0).contiguous().to(b.device, b.dtype) if dw_fn is not None else None
        return (torch.cat(packs), packs[0].numel() // 2, torch.cat([bl.to(b.device).float(), bh.to(b.device).float()]).contiguous(),
                pack_conv_weight(wz, b.dtype, b.device), wdw)

    wsub, wset, bias, wz, wdw = mod._packed(_dev_key(b, "wavelet_z"), build)
    z = L.empty_nhwc(B, c, H // 2, W // 2, b.dtype, b.device)
    M = B * (H // 2) * (W // 2)
    flops = 2.0 * M * ((c // 2) * c + 3 * (c // 2) * 9 * c + c * 2 * c) + 4.0 * b.numel()
    if k == 2 and wdw is None:
        with _tr("wavelet_z_kernel", _nb(b, z) + ((c // 2) * 10 * c + 2 * c * c) * 2, flops, note=f"C{c} {H}x{W}"):
            L.check(L.lib().ey_wavelet_z(L.dtype_code(b.dtype), B, H, W, c, b.data_ptr(), L.cstride(b), wsub.data_ptr(), wset, bias.data_ptr(), wz.data_ptr(),
                                         z.data_ptr(), L.cstride(z), L.stream()), "ey_wavelet_z")
        return z
    taps = dwt.taps(b) if k > 2 else None
    label = f"wavelet_z_kernel<k{k}{',ds' if wdw is not None else ''}>"
    with _tr(label, _nb(b, z) + ((c // 2) * 10 * c + 2 * c * c) * 2, flops, note=f"C{c} {H}x{W}"):
        L.check(L.lib().ey_wavelet_z2(L.dtype_code(b.dtype), B, H, W, c, k, _p(taps), int(wdw is not None), _p(wdw), b.data_ptr(), L.cstride(b), wsub.data_ptr(), wset,
                                      bias.data_ptr(), wz.data_ptr(), z.data_ptr(), L.cstride(z), L.stream()), "ey_wavelet_z2")
    return z


def sppf_pool(x, y1, y2, y3):
    L.require_device(x, "sppf_pool")
    B, c, H, W = x.shape
    cs = L.cstride(y1)
    if L.cstride(y2) != cs or L.cstride(y3) != cs:
        raise ValueError("sppf_pool: outputs must share one pixel stride")
    if RECORD is not None:
        RECORD.pool(x, y1, y2, y3)
        return
    with _tr("sppf_kernel", _nb(x, y1, y2, y3)):
        L.check(L.lib().ey_sppf_pool(L.dtype_code(x.dtype), B, H, W, c, x.data_ptr(), L.cstride(x), y1.data_ptr(), y2.data_ptr(), y3.data_ptr(), cs,
                                     L.stream()), "ey_sppf_pool")


def copy_slice(src, dst, up=0):
    """dst[b,c,y,x] = src[b,c,y>>up,x>>up] (both NHWC views)."""
    B, c, H, W = dst.shape
    _no_block("copy / concat / upsample")
    with _tr("copy_kernel", _nb(src, dst)):
        L.check(L.lib().ey_copy_nhwc(L.dtype_code(dst.dtype), B, H, W, c, up, src.data_ptr(), L.cstride(src), dst.data_ptr(), L.cstride(dst), L.stream()),
                "ey_copy_nhwc")
    return dst


def concat(xs):
    xs = [L.as_nhwc(as_tensor(t)) for t in xs]
    L.require_device(xs[0], "concat")
    B, _, H, W = xs[0].shape
    out = L.empty_nhwc(B, sum(t.shape[1] for t in xs), H, W, xs[0].dtype, xs[0].device)
    c0 = 0
    for t in xs:
        if (t.shape[0], t.shape[2], t.shape[3]) != (B, H, W) or t.dtype != out.dtype:
            raise ValueError(f"concat: incompatible inputs {[tuple(t.shape) for t in xs]}")
        copy_slice(t, out[:, c0:c0 + t.shape[1]])
        c0 += t.shape[1]
    return out


def upsample2x(x):
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "upsample2x")
    B, c, H, W = x.shape
    return copy_slice(x, L.empty_nhwc(B, c, 2 * H, 2 * W, x.dtype, x.device), up=1)


def to_nchw_contiguous(x):
    """NHWC view -> plain contiguous NCHW tensor (what a foreign caller expects from .contiguous())."""
    x = L.as_nhwc(x)
    B, c, H, W = x.shape
    out = torch.empty((B, c, H, W), dtype=x.dtype, device=x.device)
    L.check(L.lib().ey_nhwc_to_nchw(L.dtype_code(x.dtype), B, c, H, W, x.data_ptr(), L.cstride(x), out.data_ptr(), L.stream()), "ey_nhwc_to_nchw")
    return out


def linear_attention(qkv, heads, out=None):
    """qkv (B,3C,H,W) [q|k|v] -> (B,C,H,W)."""
    L.require_device(qkv, "linear_attention")
    qkv = L.as_nhwc(qkv)
    B, c3, H, W = qkv.shape
    c = c3 // 3
    out = _out("linear_attention: out=", out, (B, c, H, W), qkv.dtype, qkv.device)
    if RECORD is not None:
        RECORD.linattn(qkv, heads, out)
        return out
    with _tr("linattn_kernel", _nb(qkv, out), 4.0 * B * H * W * c * (c // heads)):
        L.check(L.lib().ey_linear_attention(L.dtype_code(qkv.dtype), B, H * W, c, heads, qkv.data_ptr(), L.cstride(qkv), out.data_ptr(), L.cstride(out),
                                            L.stream()), "ey_linear_attention")
    return out


def softmax_attention(qkv, heads, kd, hd, scale, out=None):
    L.require_device(qkv, "softmax_attention")
    _no_block("softmax attention")
    qkv = L.as_nhwc(qkv)
    B, _, H, W = qkv.shape
    out = _out("softmax_attention: out=", out, (B, heads * hd, H, W), qkv.dtype, qkv.device)
    with _tr("softattn_kernel", _nb(qkv, out), 2.0 * B * heads * (H * W) ** 2 * (kd + hd)):
        L.check(L.lib().ey_softmax_attention(L.dtype_code(qkv.dtype), B, H * W, heads, kd, hd, float(scale), qkv.data_ptr(), L.cstride(qkv),
                                             out.data_ptr(), L.cstride(out), L.stream()), "ey_softmax_attention")
    return out


def _group_attention(name, q, k, v, heads, area, scale, out):
    """Checks, output, trace record and call behind area_attention (ey_area_attention) and flash_attention (area None: ey_flash_attention)."""
    L.require_device(q, name)
    _no_block(name.replace("_", " "))
    q, k, v = L.as_nhwc(q), L.as_nhwc(k), L.as_nhwc(v)
    B, c, H, W = q.shape
    N = H * W
    if area and N % area:
        raise ValueError(f"{name}: {H}x{W} = {N} tokens do not split into {area} equal areas")
    if c % heads or k.shape != q.shape or v.shape != q.shape or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"{name}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, heads {heads}")
    out = _out(name + ": out=", out, q.shape, q.dtype, q.device)
    hd = c // heads
    note = f"{H}x{W} area{area} h{heads}" if area else f"{H}x{W} h{heads} hd{hd}"
    views = (float(scale), q.data_ptr(), L.cstride(q), k.data_ptr(), L.cstride(k), v.data_ptr(), L.cstride(v), out.data_ptr(), L.cstride(out), L.stream())
    rec = _tr("area_attn_kernel", _nb(q, k, v, out), 4.0 * B * heads * N * (N // (area or 1)) * hd, note=note)
    with rec:
        if area:
            rc, mfma = L.lib().ey_area_attention(L.dtype_code(q.dtype), B, N, area, heads, hd, *views), L.ATTN_AREA_MFMA
        else:
            rc, mfma = L.lib().ey_flash_attention(L.dtype_code(q.dtype), B, N, heads, hd, *views), L.ATTN_FLASH_MFMA + hd
        L.check(rc, "ey_" + name)
        if TRACE is not None and L.lib().ey_attention_last_variant() == mfma:
            rec.kernel = f"flash_attn_kernel<{hd}>"
    return out


def area_attention(q, k, v, heads, area, scale, out=None):
    """Area attention core (ey_area_attention): q, k, v (B,C,H,W) NHWC views, C = heads*head_dim -> (B,C,H,W).  The H*W tokens of an
    image, row-major, are cut into `area` equal runs attended separately; N % area != 0 is refused like the reference's reshape."""
    return _group_attention("area_attention", q, k, v, heads, area, scale, out)


def scale_add_channels(x, gamma, t, out=None):
    """out = x + gamma[c] * t (per-channel layer scale + residual, one HIP launch); gamma: device fp32 (C,)."""
    L.require_device(t, "scale_add_channels")
    _no_block("layer scale")
    x, t = L.as_nhwc(x), L.as_nhwc(t)
    B, c, H, W = t.shape
    if tuple(x.shape) != (B, c, H, W) or gamma.numel() != c or gamma.dtype != torch.float32:
        raise ValueError(f"scale_add_channels: x {tuple(x.shape)}, t {tuple(t.shape)}, gamma {tuple(gamma.shape)} {gamma.dtype}")
    out = _out("scale_add_channels: out=", out, (B, c, H, W), t.dtype, t.device)
    with _tr("scale_add_kernel", _nb(x, t, out)):
        L.check(L.lib().ey_scale_add_channels(L.dtype_code(t.dtype), B, H, W, c, x.data_ptr(), L.cstride(x), gamma.data_ptr(), t.data_ptr(),
                                              L.cstride(t), out.data_ptr(), L.cstride(out), L.stream()), "ey_scale_add_channels")
    return out


def avgpool2(x, out=None):
    """AvgPool2d(2) with floor semantics (ey_avgpool2): (B,C,H,W) -> (B,C,H//2,W//2); out= may be a channel slot of a concat buffer."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "avgpool2")
    _no_block("average pool")
    B, c, H, W = x.shape
    if H < 2 or W < 2:
        raise ValueError(f"avgpool2: a {H}x{W} map has no 2x2 window")
    out = _out("avgpool2: out=", out, (B, c, H // 2, W // 2), x.dtype, x.device)
    with _tr("avgpool2_kernel", _nb(x, out), 4.0 * out.numel(), note=f"C{c} {H}x{W}"):
        L.check(L.lib().ey_avgpool2(L.dtype_code(x.dtype), B, H, W, c, x.data_ptr(), L.cstride(x), out.data_ptr(), L.cstride(out), L.stream()),
                "ey_avgpool2")
    return out


def adown_pool(x, c_avg=None, a=None, m=None):
    """Pooling front end of ADown / AConv (ey_adown_pool): A = avg_pool2d(x, 2, 1, 0); returns (a, m) with a = A[:, :c_avg] (B,c_avg,H-1,W-1)
    and m = max_pool2d(A[:, c_avg:], 3, 2, 1) (B,C-c_avg,H//2,W//2), m None when c_avg == C (the default, AConv).  x, a= and m= may be
    channel slots of larger NHWC buffers."""
    B, c, H, W = x.shape
    c_avg = c if c_avg is None else int(c_avg)
    if H < 2 or W < 2:
        raise ValueError(f"adown_pool: a {H}x{W} map has no 2x2 window")
    if c % 8 or c_avg % 8 or not 0 < c_avg <= c:
        raise ValueError(f"adown_pool: C={c}, c_avg={c_avg}: channel counts and the split must be multiples of 8 with 0 < c_avg <= C")
    L.require_device(x, "adown_pool")
    _no_block("adown pool")
    x = L.as_nhwc(as_tensor(x))
    _nhwc_view(x, "adown_pool: x", x.shape, x.dtype, slot=True)
    a = _out("adown_pool: a=", a, (B, c_avg, H - 1, W - 1), x.dtype, x.device, slot=True)
    if c_avg == c:
        if m is not None:
            raise ValueError("adown_pool: m= given but c_avg == C leaves no channels to max-pool")
    else:
        m = _out("adown_pool: m=", m, (B, c - c_avg, H // 2, W // 2), x.dtype, x.device, slot=True)
    with _tr("adown_kernel", _nb(x, a, m), 4.0 * a.numel() + (13.0 * m.numel() if m is not None else 0.0), note=f"C{c} split{c_avg} {H}x{W}"):
        L.check(L.lib().ey_adown_pool(L.dtype_code(x.dtype), B, H, W, c, c_avg, x.data_ptr(), L.cstride(x), a.data_ptr(), L.cstride(a), *_pcs(m), L.stream()),
                "ey_adown_pool")
    return a, m


def cbfuse(xs, out=None):
    """CBFuse (ey_cbfuse): every map of `xs` (1 to 6 NHWC views with equal batch and channel counts) nearest-resized to the LAST one's size and
    summed in fp32 in list order, one rounding -> (B,C,H,W).  The maps may be channel slices of larger buffers (CBLinear's outputs)."""
    xs = list(xs)
    if not 1 <= len(xs) <= L.CBFUSE_MAX:
        raise ValueError(f"cbfuse: {len(xs)} sources; the kernel takes 1 to {L.CBFUSE_MAX}")
    if xs[-1].shape[1] % 8:
        raise ValueError(f"cbfuse: C={xs[-1].shape[1]} must be a multiple of 8")
    L.require_device(xs[-1], "cbfuse")
    _no_block("cbfuse")
    xs = [L.as_nhwc(as_tensor(t)) for t in xs]
    B, c, H, W = xs[-1].shape
    dt = xs[-1].dtype
    for i, t in enumerate(xs):
        if t.shape[0] != B or t.shape[1] != c or t.dtype != dt:
            raise ValueError(f"cbfuse: source {i} is {tuple(t.shape)} {t.dtype}, the target {tuple(xs[-1].shape)} {dt}")
        _nhwc_view(t, f"cbfuse: source {i}", t.shape, dt, slot=True)
    out = _out("cbfuse: out=", out, (B, c, H, W), dt, xs[-1].device, slot=True)
    srcs = (L.CBFuseSrc * len(xs))()
    for s, t in zip(srcs, xs):
        s.ptr, s.cstride, s.Hi, s.Wi = t.data_ptr(), L.cstride(t), t.shape[2], t.shape[3]
    with _tr("cbfuse_kernel", _nb(*xs, out), float(len(xs) - 1) * out.numel(), note=f"C{c} {H}x{W} n{len(xs)}"):
        L.check(L.lib().ey_cbfuse(L.dtype_code(dt), B, H, W, c, len(xs), ctypes.cast(srcs, ctypes.c_void_p), out.data_ptr(), L.cstride(out), L.stream()),
                "ey_cbfuse")
    return out


def dysample(mod, x, out=None):
    """DySample x2 (ey_dysample): (B,C,H,W) -> (B,C,2H,2W), offsets and bilinear gather in one launch; `mod` supplies dense_weights(),
    init_pos and groups.  out= may be a channel slot of a concat buffer."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "dysample")
    _no_block("dysample")
    B, c, H, W = x.shape
    if c != mod.in_channels:
        raise ValueError(f"dysample: input has {c} channels, the module was built for {mod.in_channels}")
    dtype, dev = x.dtype, x.device

    def build():
        w, b, s = mod.dense_weights()
        return (w.to(dev, dtype).contiguous(), b.to(dev).contiguous(), None if s is None else s.to(dev, dtype).contiguous(),
                mod.init_pos.detach().to(dev, torch.float32).flatten().contiguous())

    w, b, s, pos = mod._packed(_dev_key(x, "dysample"), build)
    out = _out("dysample: out=", out, (B, c, 2 * H, 2 * W), dtype, dev)
    flops = 2.0 * B * H * W * c * w.shape[0] * (2 if s is not None else 1) + 7.0 * out.numel()
    with _tr("dysample_kernel", _nb(x, out), flops, note=f"C{c} G{mod.groups} {H}x{W}"):
        L.check(L.lib().ey_dysample(L.dtype_code(dtype), B, H, W, c, mod.scale, mod.groups, x.data_ptr(), L.cstride(x), w.data_ptr(), b.data_ptr(),
                                    _p(s), pos.data_ptr(), out.data_ptr(), L.cstride(out), L.stream()), "ey_dysample")
    return out


def max_sigmoid_attn(e, p, guide, bias, scale, nh, out=None):
    """Max-sigmoid attention gate of YOLO-World's C2fAttn (ey_max_sigmoid_attn): e, p (B,C,H,W) NHWC views with C = 32 nh, guide (Bg, n, C)
    dense in e's dtype with Bg = 1 or B, bias fp32 (nh,), scale fp32 (nh,) or None (1.0) -> p * sigmoid(max_n(e . guide) / sqrt(32) + bias)
    * scale per pixel and head.  out= may be a channel slot of a concat buffer."""
    e, p = L.as_nhwc(as_tensor(e)), L.as_nhwc(as_tensor(p))
    L.require_device(e, "max_sigmoid_attn")
    _no_block("max_sigmoid_attn")
    B, c, H, W = e.shape
    dtype, dev = e.dtype, e.device
    if tuple(p.shape) != (B, c, H, W) or p.dtype != dtype:
        raise ValueError(f"max_sigmoid_attn: p is {tuple(p.shape)} {p.dtype}, e is {(B, c, H, W)} {dtype}")
    if guide.dim() != 3 or guide.shape[2] != c or guide.shape[0] not in (1, B) or guide.dtype != dtype or not guide.is_contiguous() or guide.device != dev:
        raise ValueError(f"max_sigmoid_attn: guide must be a contiguous (1 or {B}, n, {c}) {dtype} tensor on {dev}, got {tuple(guide.shape)} {guide.dtype}")
    out = _out("max_sigmoid_attn: out=", out, (B, c, H, W), dtype, dev)
    n = guide.shape[1]
    with _tr("max_sigmoid_attn_kernel", _nb(e, p, out, guide), 2.0 * B * H * W * c * n, note=f"C{c} n{n} {H}x{W}"):
        L.check(L.lib().ey_max_sigmoid_attn(L.dtype_code(dtype), B, H * W, nh, c // nh if nh else 0, c, n, guide.shape[0], e.data_ptr(), L.cstride(e), p.data_ptr(),
                                            L.cstride(p), guide.data_ptr(), bias.data_ptr(), _p(scale), out.data_ptr(),
                                            L.cstride(out), L.stream()), "ey_max_sigmoid_attn")
    return out


def deconv2x2(mod, x, deconv, out=None):
    """Dense nn.ConvTranspose2d(Cin, Cout, 2, 2, 0, bias=True) (ey_deconv2x2): (B,Cin,H,W) -> (B,Cout,2H,2W) in one launch; `mod` caches the
    packed weight, `deconv` holds the parameters (Proto.upsample, reference block.py:123)."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "deconv2x2")
    _no_block("deconv2x2")
    B, cin, H, W = x.shape
    if (deconv.kernel_size != (2, 2) or deconv.stride != (2, 2) or deconv.groups != 1 or deconv.padding != (0, 0) or deconv.output_padding != (0, 0)
            or deconv.dilation != (1, 1) or deconv.in_channels != cin):
        raise NotImplementedError(f"deconv2x2: the kernel takes a dense ConvTranspose2d({cin}, Cout, 2, 2, 0), got {deconv}")
    cout, dtype, dev = deconv.out_channels, x.dtype, x.device
    if cin % 8 or cout % 8 or cin > 384 or cout > 384:
        raise NotImplementedError(f"deconv2x2: Cin={cin} Cout={cout} (multiples of 8 up to 384 are built)")

    def build():
        code = L.dtype_code(dtype)
        w = deconv.weight.detach().float().cpu().contiguous()
        nbytes = L.lib().ey_deconv2x2_packed_bytes(code, cin, cout)
        buf = torch.empty(nbytes, dtype=torch.uint8)
        L.check(L.lib().ey_deconv2x2_pack_weight(code, cin, cout, w.data_ptr(), buf.data_ptr(), nbytes), "deconv2x2_pack_weight")
        b = deconv.bias.detach().float() if deconv.bias is not None else torch.zeros(cout)
        return buf.to(dev), b.to(dev).contiguous()

    wp, bias = mod._packed(_dev_key(x, "deconv2x2"), build)
    out = _out("deconv2x2: out=", out, (B, cout, 2 * H, 2 * W), dtype, dev)
    with _tr("deconv2x2_kernel", _nb(x, out) + wp.numel(), 8.0 * B * H * W * cin * cout, note=f"C{cin}->{cout} {H}x{W}"):
        L.check(L.lib().ey_deconv2x2(L.dtype_code(dtype), B, H, W, cin, cout, x.data_ptr(), L.cstride(x), wp.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                     L.cstride(out), L.stream()), "ey_deconv2x2")
    return out


def _mask_assembly(what, proto, coefs, rows, boxes, N):
    """What process_mask and process_mask_native check and build alike: proto and every coefficient map are NHWC views, the maps have proto's
    batch and channel counts and one dtype, rows is a dense int32 (>= N, 2) and boxes a dense fp32 (>= N, 4) tensor on proto's device.
    -> the leading arguments of both entry points, up to the boxes' pointer."""
    _nhwc_view(proto, f"{what}: proto", proto.shape, proto.dtype)
    B, nm, mh, mw = proto.shape
    for i, c in enumerate(coefs):
        _nhwc_view(c, f"{what}: coefs[{i}]", (B, nm, *c.shape[2:]), coefs[0].dtype)
    _dense(rows, f"{what}: rows", torch.int32, (_AtLeast(N), 2), proto.device)
    _dense(boxes, f"{what}: boxes", torch.float32, (_AtLeast(N), 4), proto.device)
    return (L.dtype_code(proto.dtype), B, mh, mw, nm, proto.data_ptr(), L.cstride(proto), len(coefs), _pa(coefs), L.dtype_code(coefs[0].dtype) if coefs else L.F32,
            _ia(L.cstride(c) for c in coefs), _ia(c.shape[2] for c in coefs), _ia(c.shape[3] for c in coefs), N, rows.data_ptr(), boxes.data_ptr())


def process_mask(proto, coefs, rows, boxes, s, n=None, out=None):
    """Mask assembly (ey_process_mask): proto logical (B,nm,mh,mw) NHWC view; coefs: list (<= 4) of logical (B,nm,H_l,W_l) NHWC views in
    concatenated-anchor order; rows int32 (N,2) = (image, anchor); boxes fp32 (N,4) xyxy in network-input pixels; s = input / proto ratio.
    -> uint8 (N, s*mh, s*mw), values 0 / 1.  n: number of leading rows to use (default all); out=: a contiguous uint8 buffer to fill."""
    L.require_device(proto, "process_mask")
    _no_block("process_mask")
    N = int(rows.shape[0]) if n is None else int(n)
    head = _mask_assembly("process_mask", proto, coefs, rows, boxes, N)
    _, nm, mh, mw = proto.shape
    s = int(s)
    out = _dense_out("process_mask: out=", out, torch.uint8, (N, s * mh, s * mw), proto.device)
    with _tr("process_mask_kernel", out.numel() + N * 24 + _nb(proto), 2.0 * N * mh * mw * nm, note=f"N{N} {mh}x{mw} s{s}"):
        L.check(L.lib().ey_process_mask(*head, s, out.data_ptr(), L.stream()), "ey_process_mask")
    return out


def mask_iou(pred, pred_off, gt, gt_off, index=False, out_off=None, iou=None, inter=None, workspace=None):
    """Mask IoU of a batch (ey_mask_iou): pred uint8 (N_total,H,W) 0/1 grouped by image through the host list pred_off (B+1 entries);
    gt either a uint8 stack (M_total,H,W) grouped by gt_off, or with index=True one int32 map (B,H,W) per image whose instance m is the
    pixels equal to m+1 (gt_off still gives the instance counts).  Image b's row-major [M_b][N_b] matrix lands at element out_off[b] of the
    flat fp32 buffer `iou` (and of the int32 buffer `inter`, True = allocate one); by default the matrices are packed one after the other.
    -> (iou, out_off, inter or None); the matrices: iou[out_off[b]: out_off[b] + M_b * N_b].view(M_b, N_b)."""
    L.require_device(pred, "mask_iou")
    _no_block("mask_iou")
    pred_off, gt_off, out_off, sizes, end = _pair_offsets("mask_iou", pred_off, gt_off, out_off)
    B, dev = len(out_off), pred.device
    _dense(pred, "mask_iou: pred", torch.uint8, (_AtLeast(pred_off[-1]), _ANY, _ANY), dev)
    H, W = int(pred.shape[1]), int(pred.shape[2])
    _dense(gt, "mask_iou: gt", torch.int32 if index else torch.uint8, (_AtLeast(B if index else gt_off[-1]), H, W), dev)
    iou = _dense_out("mask_iou: iou", iou, torch.float32, (_AtLeast(end),), dev)
    if inter is not None:
        inter = _dense_out("mask_iou: inter", None, torch.int32, (iou.numel(),), dev) if inter is True else _dense(inter, "mask_iou: inter", torch.int32, (_AtLeast(end),), dev)
    workspace = _workspace("mask_iou", workspace, L.lib().ey_mask_iou_workspace_bytes(H, W, pred_off[-1], gt_off[-1]), dev)
    words = (H * W + 63) // 64
    with _tr("mask_iou_kernels", pred_off[-1] * H * W + gt.numel() * gt.element_size() + 8 * end, 2.0 * sum(sizes) * words,
             note=f"B{B} N{pred_off[-1]} M{gt_off[-1]} {H}x{W}", kernels=3):
        L.check(L.lib().ey_mask_iou(L.MASK_GT_INDEX if index else L.MASK_GT_STACK, B, H, W, pred.data_ptr(), _ia(pred_off), gt.data_ptr(), _ia(gt_off),
                                    _la(out_off), iou.data_ptr(), _p(inter), workspace.data_ptr(), workspace.numel(),
                                    L.stream()), "ey_mask_iou")
    return iou, out_off, inter


def mask_geometry(mask_hw, shape, padding=True):
    """The crop and target of scale_masks (reference utils/ops.py:726-733, the same Python float arithmetic) as the record ey_mask_prompt
    and ey_scale_masks take: (top, bottom, left, right, H0, W0).  padding=False: the crop starts at the top-left corner and the whole
    padding comes off the bottom and the right (the reference halves `pad` only with padding=True and subtracts it either way)."""
    mh, mw = int(mask_hw[0]), int(mask_hw[1])
    h0, w0 = int(shape[0]), int(shape[1])
    gain = min(mh / h0, mw / w0)
    pad = [mw - w0 * gain, mh - h0 * gain]
    if padding:
        pad[0] /= 2
        pad[1] /= 2
    top, left = (int(pad[1]), int(pad[0])) if padding else (0, 0)
    return (top, int(mh - pad[1]), left, int(mw - pad[0]), h0, w0)


def process_mask_native(proto, coefs, rows, boxes, mask_off, shapes, out=None):
    """Mask assembly at the original resolution (ey_process_mask_native): proto, coefs and rows as for process_mask; boxes fp32 (N,4) xyxy
    in ORIGINAL-image pixels of the row's image (after scale_boxes); mask_off: host list, B+1 entries, image b owns rows mask_off[b] ..
    mask_off[b+1]-1; shapes: the B original (H0, W0), which may all differ.  -> (flat, views): one flat uint8 buffer and image b's masks as
    its (n_b, H0_b, W0_b) view, values 0 / 1, one after the other.  out=: a flat contiguous uint8 buffer of at least that many bytes to
    fill (its first sum n_b H0_b W0_b bytes are written)."""
    L.require_device(proto, "process_mask_native")
    _no_block("process_mask_native")
    B, nm, mh, mw = proto.shape
    mask_off = [int(v) for v in mask_off]
    if len(mask_off) != B + 1 or len(shapes) != B or mask_off[0] != 0:
        raise ValueError(f"process_mask_native: mask_off must have B+1 = {B + 1} entries starting at 0 and shapes B entries")
    N = mask_off[-1]
    head = _mask_assembly("process_mask_native", proto, coefs, rows, boxes, N)
    if any(int(s[0]) < 1 or int(s[1]) < 1 for s in shapes):
        raise ValueError(f"process_mask_native: original shapes {[tuple(s) for s in shapes]} must be at least 1 x 1")
    geo = [mask_geometry((mh, mw), s) for s in shapes]
    counts = [mask_off[b + 1] - mask_off[b] for b in range(B)]
    out_off, total = [], 0
    for k, g in zip(counts, geo):
        out_off.append(total)
        total += max(k, 0) * max(g[4], 0) * max(g[5], 0)
    out = _dense_out("process_mask_native: out=", out, torch.uint8, (_AtLeast(total),), proto.device)
    with _tr("process_mask_native_kernel", total + N * 24 + _nb(proto), 2.0 * N * mh * mw * nm, note=f"B{B} N{N} {mh}x{mw} -> {sorted(set(map(tuple, shapes)))}"):
        rc = L.lib().ey_process_mask_native(*head, _ia(mask_off), _ia(v for g in geo for v in g), _la(out_off), out.data_ptr(), L.stream())
        if rc == -1:  # EY_EINVAL: a bad argument of the caller's (an empty crop, offsets that do not group the rows)
            raise ValueError("ey_process_mask_native: " + L.lib().ey_last_error().decode(errors="replace"))
        L.check(rc, "ey_process_mask_native")
    views = [out[o:o + k * g[4] * g[5]].view(k, g[4], g[5]) if k > 0 else out[:0].view(0, max(g[4], 0), max(g[5], 0)) for o, k, g in zip(out_off, counts, geo)]
    return out, views


def mask_prompt(masks, mask_off, shapes, bboxes=None, points=None, labels=None, out=None, workspace=None):
    """FastSAM prompt selection of a batch (ey_mask_prompt): masks uint8 (N,mh,mw) 0/1 grouped by image through the host list mask_off
    (B+1 entries); shapes: the B original (H0, W0); bboxes: P host rows x1,y1,x2,y2 and points: Q host rows x,y with `labels`, int, in
    original-image pixels, shared by all images.  -> dict(full (N,), inter / iou (P,N), best int32 (B,P), hit uint8 (Q,N), keep uint8 (N,)).
    out=: a dict of buffers to write instead (full, keep, and inter / iou / best / hit as the prompts need them; inter, iou and hit may be
    wider than N: their row stride is taken from `inter`, else `hit`)."""
    L.require_device(masks, "mask_prompt")
    _no_block("mask_prompt")
    mask_off = [int(v) for v in mask_off]
    B = len(mask_off) - 1
    if B < 0 or mask_off[0] != 0 or len(shapes) != B:
        raise ValueError("mask_prompt: mask_off must have B+1 entries starting at 0 and shapes B entries")
    N = mask_off[-1]
    dev = masks.device
    _dense(masks, "mask_prompt: masks", torch.uint8, (_AtLeast(N), _ANY, _ANY), dev)
    mh, mw = int(masks.shape[1]), int(masks.shape[2])
    boxes = [[int(v) for v in r] for r in ([] if bboxes is None else bboxes)]
    pts = [[int(v) for v in r] for r in ([] if points is None else points)]
    labs = [1] * len(pts) if labels is None else [int(v) for v in labels]
    if any(len(r) != 4 for r in boxes) or any(len(r) != 2 for r in pts) or len(labs) != len(pts):
        raise ValueError(f"mask_prompt: boxes must be (P,4), points (Q,2) and labels (Q,); got {len(pts)} points and {len(labs)} labels")
    P, Q = len(boxes), len(pts)
    want = {"full": ((N,), torch.float32), "keep": ((N,), torch.uint8)}
    if P:
        want.update(inter=((P, N), torch.float32), iou=((P, N), torch.float32), best=((B, P), torch.int32))
    if Q:
        want["hit"] = ((Q, N), torch.uint8)
    ld = N
    if out is None:
        out = {k: torch.empty(s, dtype=dt, device=dev) for k, (s, dt) in want.items()}
    else:  # inter, iou and hit share the row stride of the first of them; one that is narrower than N or not 2-D fails its check below
        lead = out.get("inter" if P else "hit")
        ld = max(int(lead.shape[1]), N) if torch.is_tensor(lead) and lead.dim() == 2 else N
        for k, (s, dt) in want.items():
            _dense(out.get(k), f"mask_prompt: out['{k}']", dt, (s[0], ld) if k in ("inter", "iou", "hit") else s, dev)
    workspace = _workspace("mask_prompt", workspace, L.lib().ey_mask_prompt_workspace_bytes(B, mh, mw, min(P, 32)), dev)
    geo = [v for s in shapes for v in mask_geometry((mh, mw), s)]
    with _tr("mask_prompt_kernels", N * mh * mw + 4 * N * (2 * P + 1) + N * (Q + 1), 2.0 * N * mh * mw * (P + 1), note=f"B{B} N{N} P{P} Q{Q} {mh}x{mw}", kernels=3):
        L.check(L.lib().ey_mask_prompt(B, mh, mw, masks.data_ptr(), _ia(mask_off), _ia(geo), P, _ia(v for r in boxes for v in r), Q, _ia(v for r in pts for v in r),
                                       _ia(labs), ld, out["full"].data_ptr(), _p(out.get("inter") if P else None), _p(out.get("iou") if P else None),
                                       _p(out.get("best") if P else None), _p(out.get("hit") if Q else None), out["keep"].data_ptr(), workspace.data_ptr(),
                                       workspace.numel(), L.stream()), "ey_mask_prompt")
    return out


def scale_masks(masks, shape, padding=True, out=None):
    """ey_scale_masks: (N,C,H,W) uint8 / f16 / fp32 -> (N,C,*shape), fp32 for uint8 input, else the input's dtype (reference utils/ops.py:716-737)."""
    L.require_device(masks, "scale_masks")
    _no_block("scale_masks")
    if masks.dim() != 4 or masks.dtype not in (torch.uint8, torch.float16, torch.float32, torch.bool):
        raise ValueError(f"scale_masks: masks must be an (N,C,H,W) uint8, bool, float16 or float32 tensor, got {masks.dtype} {tuple(masks.shape)}")
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    masks = masks.contiguous()
    n, c, h, w = (int(v) for v in masks.shape)
    h0, w0 = int(shape[0]), int(shape[1])
    top, bottom, left, right = mask_geometry((h, w), shape, padding)[:4]
    odt = torch.float32 if masks.dtype == torch.uint8 else masks.dtype
    out = _dense_out("scale_masks: out=", out, odt, (n, c, h0, w0), masks.device)
    code = L.MASK_U8 if masks.dtype == torch.uint8 else L.dtype_code(masks.dtype)
    with _tr("scale_masks_kernel", _nb(masks, out), 7.0 * out.numel(), note=f"{n * c} x {h}x{w}->{h0}x{w0}"):
        L.check(L.lib().ey_scale_masks(code, n * c, h, w, top, bottom, left, right, h0, w0, masks.data_ptr(), out.data_ptr(), L.stream()), "ey_scale_masks")
    return out


def dwconv_s2(mod, x, folded_fn, k, act, out=None, tag="dw2"):
    """Depthwise kxk, stride 2, pad k//2 (ey_dwconv_s2): the depthwise half of DSConv(c, c, k, 2)."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "dwconv_s2")
    _no_block("stride-2 depthwise conv")
    B, c, H, W = x.shape
    wk, bias = _dw_pack(mod, x, folded_fn, c, k, tag)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = _out("dwconv_s2: out=", out, (B, c, Ho, Wo), x.dtype, x.device)
    with _tr(f"dwconv_s2_kernel<{k}>", _nb(x, out), 2.0 * B * Ho * Wo * c * k * k, note=f"C{c} {H}x{W}"):
        L.check(L.lib().ey_dwconv_s2(L.dtype_code(x.dtype), B, H, W, c, k, act, x.data_ptr(), L.cstride(x), wk.data_ptr(), _p(bias), out.data_ptr(), L.cstride(out),
                                     L.stream()), "ey_dwconv_s2")
    return out


HG_CONTEXT = {"both": 0, "mean": 1, "max": 2}
HG_LAUNCHES = 5  # kernels behind one ey_hypergraph_conv call


def hypergraph_conv(mod, x, out=None):
    """AdaHGConv on the H*W tokens of each image of x (B,D,H,W) (ey_hypergraph_conv) -> (B,D,H,W).  mod: the AdaHGConv (weights are
    packed once per dtype / device; the workspace is cached per shape, so a captured graph replays with no host work)."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "hypergraph_conv")
    _no_block("hypergraph convolution")
    B, D, H, W = x.shape
    N = H * W
    g = mod.edge_generator
    E = g.num_hyperedges
    if D != g.prototype_base.shape[1]:
        raise ValueError(f"hypergraph_conv: input has {D} channels, the module {g.prototype_base.shape[1]}")
    half = x.dtype == torch.float16

    def build():
        f = lambda t: t.detach().float().to(x.device).contiguous()  # noqa: E731
        nw = mod.node_proj[0].weight.detach().float()
        if half:
            kp = (D + 31) // 32 * 32
            wn = torch.zeros((D, kp), dtype=torch.float16)
            wn[:, :D] = nw.cpu().half()
            wn = wn.to(x.device)
        else:
            wn = f(nw.t())
        return (f(g.prototype_base), f(g.context_net.weight.t()), f(g.context_net.bias), f(g.pre_head_proj.weight), f(g.pre_head_proj.bias),
                f(mod.edge_proj[0].weight.t()), f(mod.edge_proj[0].bias), wn, f(mod.node_proj[0].bias))

    w = mod._packed(_dev_key(x, "hypergraph"), build)
    nbytes = L.lib().ey_hypergraph_workspace_bytes(B, N, D, E)
    ws = mod._packed(("hg_ws", B, N, D, x.device), lambda: torch.empty(nbytes, dtype=torch.uint8, device=x.device))
    out = _out("hypergraph_conv: out=", out, (B, D, H, W), x.dtype, x.device)
    flops = 2.0 * B * N * D * (E * 3 + D) + 2.0 * B * E * D * (D * 2 + (2 if g.context == "both" else 1) * D)
    with _tr("hypergraph_kernels", _nb(x, x, x, out) + 8.0 * B * N * E, flops, note=f"{H}x{W} D{D} E{E}", kernels=HG_LAUNCHES):
        L.check(L.lib().ey_hypergraph_conv(L.dtype_code(x.dtype), B, N, D, E, g.num_heads, HG_CONTEXT[g.context], x.data_ptr(), L.cstride(x), out.data_ptr(),
                                           L.cstride(out), *[t.data_ptr() for t in w], ws.data_ptr(), ws.numel(), L.stream()), "ey_hypergraph_conv")
    return out


# ----------------------------------------------------------------------------------------------- LGL block (YOLOv13 DSC3K2_LGL)
def flash_attention(q, k, v, heads, scale, out=None):
    """Softmax attention over all H*W tokens of each image (ey_flash_attention): q, k, v (B,C,H,W) NHWC views, C = heads*head_dim."""
    return _group_attention("flash_attention", q, k, v, heads, None, scale, out)


def dwconv_gate(mod, x, conv, mode, out=None, tag=""):
    """Depthwise kxk + bias of the nn.Conv2d `conv` (k 3 or 9) with the epilogue `mode` (L.DWG_PLAIN / _GATE / _RESIDUAL), ey_dwconv_gate."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "dwconv_gate")
    _no_block("gated depthwise conv")
    B, c, H, W = x.shape
    k = conv.kernel_size[0]
    wk, bias = _dw_pack(mod, x, lambda: (conv.weight.detach().float(), None if conv.bias is None else conv.bias.detach()), c, k, "dwg" + tag)
    out = _out("dwconv_gate: out=", out, x.shape, x.dtype, x.device)
    with _tr(f"lgl_dw_kernel<{k}>", _nb(x, out), 2.0 * x.numel() * k * k, note=f"C{c} {H}x{W} mode{mode}"):
        L.check(L.lib().ey_dwconv_gate(L.dtype_code(x.dtype), B, H, W, c, k, mode, x.data_ptr(), L.cstride(x), wk.data_ptr(), _p(bias), out.data_ptr(), L.cstride(out),
                                       L.stream()), "ey_dwconv_gate")
    return out


def sigmoid_gate(x, g, out=None):
    """out = x + x * (sigmoid(g) - 1/2) (ey_sigmoid_gate)."""
    x, g = L.as_nhwc(as_tensor(x)), L.as_nhwc(g)
    L.require_device(x, "sigmoid_gate")
    _no_block("sigmoid gate")
    B, c, H, W = x.shape
    if g.shape != x.shape or g.dtype != x.dtype:
        raise ValueError(f"sigmoid_gate: x {tuple(x.shape)} {x.dtype}, g {tuple(g.shape)} {g.dtype}")
    out = _out("sigmoid_gate: out=", out, x.shape, x.dtype, x.device)
    with _tr("lgl_gate_kernel", _nb(x, g, out), 4.0 * x.numel()):
        L.check(L.lib().ey_sigmoid_gate(L.dtype_code(x.dtype), B, H, W, c, x.data_ptr(), L.cstride(x), g.data_ptr(), L.cstride(g), out.data_ptr(),
                                        L.cstride(out), L.stream()), "ey_sigmoid_gate")
    return out


def gelu(x, out=None):
    """Exact (erf) GELU (ey_gelu); out= may be x itself."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "gelu")
    _no_block("GELU")
    B, c, H, W = x.shape
    out = _out("gelu: out=", out, x.shape, x.dtype, x.device)
    with _tr("lgl_gelu_kernel", _nb(x, out), 8.0 * x.numel()):
        L.check(L.lib().ey_gelu(L.dtype_code(x.dtype), B, H, W, c, x.data_ptr(), L.cstride(x), out.data_ptr(), L.cstride(out), L.stream()), "ey_gelu")
    return out


def cmlp(mod, x, fc1, fc2, bn=None, gate=False, out=None):
    """fc2(GELU(fc1(bn(x)))) of a CMlp whose convs are grouped per channel (ey_cmlp), optionally gated: x + x * (sigmoid(.) - 1/2).
    mod: the module caching the packed weights; fc1 / fc2: nn.Conv2d(C, rC, 3, 1, 1, groups=C) / (rC, C, 3, 1, 1, groups=C)."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "cmlp")
    _no_block("CMlp")
    B, c, H, W = x.shape
    hid = fc1.out_channels
    if (fc1.groups != c or fc2.groups != c or fc1.in_channels != c or fc2.out_channels != c or hid % c or fc2.in_channels != hid
            or fc1.kernel_size != (3, 3) or fc2.kernel_size != (3, 3) or fc1.padding != (1, 1) or fc2.padding != (1, 1)):
        raise NotImplementedError("cmlp: the kernel takes Conv2d(C, rC, 3, pad 1, groups=C) -> GELU -> Conv2d(rC, C, 3, pad 1, groups=C)")
    r = hid // c

    def build():
        f = lambda t: t.detach().float().to(x.device).contiguous()  # noqa: E731
        w1 = fc1.weight.detach().float().view(c, r, 9).permute(1, 2, 0)  # [r][9][C]: grouped-conv taps per expansion channel, fp32 with their own bias layout -- not a _dw_pack
        w2 = fc2.weight.detach().float().view(c, r, 9).permute(1, 2, 0)
        b1 = fc1.bias.detach().float().view(c, r).t() if fc1.bias is not None else torch.zeros(r, c)
        b2 = fc2.bias.detach().float() if fc2.bias is not None else torch.zeros(c)
        if bn is None:
            return None, None, f(w1), f(b1), f(w2), f(b2)
        s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        return f(s), f(bn.bias.detach().float() - bn.running_mean.detach().float() * s), f(w1), f(b1), f(w2), f(b2)

    sc, sh, w1, b1, w2, b2 = mod._packed(_dev_key(x, "cmlp"), build)
    out = _out("cmlp: out=", out, x.shape, x.dtype, x.device)
    with _tr("lgl_cmlp_kernel", _nb(x, out), 2.0 * x.numel() * r * 9 * 10, note=f"C{c} r{r} {H}x{W}"):
        L.check(L.lib().ey_cmlp(L.dtype_code(x.dtype), B, H, W, c, r, int(bool(gate)), x.data_ptr(), L.cstride(x), _p(sc), _p(sh), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                b2.data_ptr(), out.data_ptr(), L.cstride(out), L.stream()), "ey_cmlp")
    return out


def _ln_params(mod, x, ln, tag):
    c = x.shape[1]
    if tuple(ln.normalized_shape) != (c,):
        raise ValueError(f"layernorm: nn.LayerNorm{tuple(ln.normalized_shape)} on {c} channels")

    def build():
        w = ln.weight.detach().float() if ln.weight is not None else torch.ones(c)
        b = ln.bias.detach().float() if ln.bias is not None else torch.zeros(c)
        return w.to(x.device).contiguous(), b.to(x.device).contiguous()

    return mod._packed(_dev_key(x, "ln" + tag), build)


def layernorm_channels(mod, x, ln, pool=False, out=None, tag=""):
    """nn.LayerNorm `ln` over the channels of each pixel of x (B,C,H,W) (ey_layernorm_channels); pool: followed by the ceil-mode 2x2
    average pool in the same kernel -> (B,C,ceil(H/2),ceil(W/2))."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "layernorm_channels")
    _no_block("LayerNorm")
    B, c, H, W = x.shape
    g, b = _ln_params(mod, x, ln, tag)
    out = _out("layernorm_channels: out=", out, (B, c, (H + 1) // 2, (W + 1) // 2) if pool else x.shape, x.dtype, x.device)
    with _tr("lgl_layernorm_kernel", _nb(x, out), 8.0 * x.numel(), note=f"C{c} {H}x{W}{' +pool' if pool else ''}"):
        L.check(L.lib().ey_layernorm_channels(L.dtype_code(x.dtype), B, H, W, c, float(ln.eps), int(bool(pool)), x.data_ptr(), L.cstride(x), g.data_ptr(),
                                              b.data_ptr(), out.data_ptr(), L.cstride(out), L.stream()), "ey_layernorm_channels")
    return out


def unpool2_layernorm(mod, t, deconv, ln, H, W, out=None, tag="up"):
    """LayerNorm(resize(ConvTranspose2d_{k2,s2,depthwise}(t))) (ey_unpool2_layernorm): t (B,C,ceil(H/2),ceil(W/2)) -> (B,C,H,W)."""
    t = L.as_nhwc(as_tensor(t))
    L.require_device(t, "unpool2_layernorm")
    _no_block("un-pool + LayerNorm")
    B, c, Hs, Ws = t.shape
    if (deconv.kernel_size != (2, 2) or deconv.stride != (2, 2) or deconv.groups != c or deconv.in_channels != c or deconv.out_channels != c
            or deconv.bias is not None or deconv.padding != (0, 0) or deconv.output_padding != (0, 0)):
        raise NotImplementedError("unpool2_layernorm: the kernel takes a depthwise ConvTranspose2d(C, C, 2, 2, groups=C, bias=False)")
    g, b = _ln_params(mod, t, ln, tag)
    # the transposed conv's 2x2 taps [a][b][C], kept in fp32 and without a bias: not a _dw_pack
    w = mod._packed(_dev_key(t, "unpool" + tag), lambda: deconv.weight.detach().float().view(c, 2, 2).permute(1, 2, 0).contiguous().to(t.device))
    out = _out("unpool2_layernorm: out=", out, (B, c, H, W), t.dtype, t.device)
    with _tr("lgl_unpool_ln_kernel", _nb(t, out), 10.0 * out.numel(), note=f"C{c} {Hs}x{Ws}->{H}x{W}"):
        L.check(L.lib().ey_unpool2_layernorm(L.dtype_code(t.dtype), B, Hs, Ws, H, W, c, float(ln.eps), t.data_ptr(), L.cstride(t), w.data_ptr(), g.data_ptr(),
                                             b.data_ptr(), out.data_ptr(), L.cstride(out), L.stream()), "ey_unpool2_layernorm")
    return out


def head_decode(box, cls, stride, q, pred, a_off):
    """One pyramid level of the fused DGQP + DFL + decode; q = (w1[hid,20], b1, w2[hid], b2) fp32 device tensors or None."""
    L.require_device(box, "head_decode")
    _no_block("head decode")
    B, _, H, W = box.shape
    nc = cls.shape[1]
    qa = [t.data_ptr() for t in q] if q is not None else [None] * 4
    hid = q[0].shape[0] if q is not None else 0
    with _tr("head_decode_kernel", _nb(box, cls) + B * H * W * (4 + nc) * 4, 2.0 * B * H * W * (hid * 21 + 200)):
        L.check(L.lib().ey_head_decode(L.dtype_code(box.dtype), B, H, W, nc, float(stride), box.data_ptr(), L.cstride(box), cls.data_ptr(), L.cstride(cls),
                                       qa[0], qa[1], qa[2], qa[3], hid, pred.data_ptr(), pred.shape[2], a_off, L.stream()), "ey_head_decode")


class Candidates:
    """NMS candidates written by the fused head decode (ey_head_decode_levels_nms): sort keys + best class per anchor + (cx,cy,w,h),
    for the conf threshold / class filter they were built with.  `utils.ops.nms_device` accepts it in place of `pred`."""

    def __init__(self, buf, B, nc, A, conf, classes, pred=None):
        self.buf, self.B, self.nc, self.A, self.conf, self.classes, self.pred = buf, B, nc, A, float(conf), (tuple(classes) if classes is not None else None), pred
        self.shape = (B, 4 + nc, A)
        self.device = buf.device


def nms_candidates(cand, iou_thres, max_det, max_nms, max_wh, agnostic):
    """Selection + greedy suppression on a Candidates buffer -> (boxes (B,max_det,6), count (B,), index (B,max_det))."""
    boxes, count, index = _nms_out(cand.B, max_det, 6, cand.device)
    # predict mode = the three-kernel fast path (csrc/nms_fast.inc.h), bracketed as one operator
    alg = cand.B * ((cand.A + 255) // 256 * 256 * 12 + cand.A * 16)  # keys + class ids + boxes (the tail of the buffer is scratch)
    with _tr("nms_fast(nf_select+nf_mask+nf_resolve)", alg + _nb(boxes), kernels=3):
        L.check(L.lib().ey_nms_candidates(cand.B, cand.nc, cand.A, cand.buf.data_ptr(), cand.buf.numel(), float(iou_thres), int(max_det), int(max_nms), float(max_wh),
                                          int(bool(agnostic)), boxes.data_ptr(), count.data_ptr(), index.data_ptr(), L.stream()), "ey_nms_candidates")
    return boxes, count, index


def _level_arrays(levels, nmaps, stride_i, off_i):
    """The ctypes arrays a per-level launch takes.  levels: one tuple per pyramid level that starts with `nmaps` NHWC views and holds the level's
    stride at index `stride_i` and its anchor offset at `off_i` -> (Hs, Ws, strides, offsets) with the sizes of map 0, [pointers of map j],
    [pixel strides of map j]."""
    grid = _ia(lv[0].shape[2] for lv in levels), _ia(lv[0].shape[3] for lv in levels), _fa(float(lv[stride_i]) for lv in levels), _ia(int(lv[off_i]) for lv in levels)
    return grid, [_pa(lv[j] for lv in levels) for j in range(nmaps)], [_ia(L.cstride(lv[j]) for lv in levels) for j in range(nmaps)]


# One pyramid level of the head decode: box / class maps (NHWC views), the level's stride, its DGQP weights (w1, b1, w2, b2) or None, and the
# index of its first anchor.  A plain 5-tuple in this order is accepted wherever a Level is.
Level = collections.namedtuple("Level", "box cls stride q a_off")


def _quality_arrays(levels):
    """Four pointer arrays of the levels' DGQP weights q = (w1, b1, w2, b2) or None."""
    return [_pa(None if lv.q is None else lv.q[j] for lv in levels) for j in range(4)]


def _decode_prologue(levels, what, cand):
    """What head_decode_levels and head_tail_decode_levels set up alike -> (levels as Level, B, hid, level arrays, quality arrays, A,
    bytes of the candidate buffer, the buffer); the last two are 0 / None unless `cand`."""
    levels = [Level(*lv) for lv in levels]
    box0, q0 = levels[0].box, levels[0].q
    L.require_device(box0, what)
    B = box0.shape[0]
    hid = q0[0].shape[0] if q0 is not None else 0
    arrays = _level_arrays([(lv.box, lv.cls, lv.stride, lv.a_off) for lv in levels], 2, 2, 3)
    A = sum(lv.box.shape[2] * lv.box.shape[3] for lv in levels)
    nb = L.lib().ey_nms_candidates_bytes(B, A) if cand else 0
    buf = torch.empty(nb, dtype=torch.uint8, device=box0.device) if cand else None
    return levels, B, hid, arrays, _quality_arrays(levels), A, nb, buf


def head_decode_levels(levels, pred, nms=None, xyxy=False):
    """levels: list (<= 4) of (box, cls, stride, q-or-None, a_off) -> every level of the fused DGQP + DFL + decode in ONE launch.
    nms = (conf_thres, class_mask uint8 tensor or None, classes): also build the NMS candidates in the same pass (pred may then be None);
    returns a Candidates object.  xyxy: rows 0-3 = x1,y1,x2,y2 (end2end heads, reference head.py:163-165)."""
    levels, B, hid, ((Hs, Ws, st, offs), (boxp, clsp), (boxcs, clscs)), qa, A, nb, buf = _decode_prologue(levels, "head_decode", nms is not None)
    n, dt, nc = len(levels), L.dtype_code(levels[0].box.dtype), levels[0].cls.shape[1]
    in_bytes = sum(_nb(lv.box, lv.cls) for lv in levels)
    flops = sum(2.0 * B * lv.box.shape[2] * lv.box.shape[3] * (hid * 21 + 200) for lv in levels)
    if nms is not None:
        conf, mask, classes = nms
        with _tr("head_decode_kernel", in_bytes + nb + (B * A * (4 + nc) * 4 if pred is not None else 0), flops, note=f"{n} levels + NMS keys"):
            L.check(L.lib().ey_head_decode_levels_nms(dt, B, n, Hs, Ws, st, boxp, boxcs, clsp, clscs, nc, qa[0], qa[1], qa[2], qa[3], hid,
                                                      _p(pred), A, offs, float(conf), _p(mask), buf.data_ptr(), nb, L.stream()), "ey_head_decode_levels_nms")
        return Candidates(buf, B, nc, A, conf, classes, pred)
    with _tr("head_decode_kernel", in_bytes + B * A * (4 + nc) * 4, flops, note=f"{n} levels"):
        fn = L.lib().ey_head_decode_levels_xyxy if xyxy else L.lib().ey_head_decode_levels
        L.check(fn(dt, B, n, Hs, Ws, st, boxp, boxcs, clsp, clscs, nc, qa[0], qa[1], qa[2], qa[3], hid,
                   pred.data_ptr(), pred.shape[2], offs, L.stream()), "ey_head_decode_levels")


def head_tail_decode_levels(levels, tails, pred, nms):
    """head_decode_levels(nms=...) with the towers' closing 1x1 convs inside the decode kernel (ey_head_tail_decode_levels_nms).
    levels: list (<= 4) of (box_feat, cls_in, stride, q-or-None, a_off); tails: per level (box_wp, box_b, chain) with chain =
    (w1p, b1, w2p, b2) -- cls_in is then the class-tower feature in front of the chain -- or None on every level (cls_in = the
    class logits).  nc: tails' class count = `nms[3]`.  Returns a Candidates object, or None when the shapes are outside the fused
    kernel (nothing launched: the caller runs the convs and head_decode_levels)."""
    _no_block("head decode")
    levels, B, hid, ((Hs, Ws, st, offs), (boxp, clsp), (boxcs, clscs)), qa, A, nb, buf = _decode_prologue(levels, "head_tail_decode", True)
    conf, mask, classes, nc = nms
    n, box0 = len(levels), levels[0].box
    fuse_cls = tails[0][2] is not None
    clscin = _ia(lv.cls.shape[1] for lv in levels)
    bw, bb = _pa(t[0] for t in tails), _pa(t[1] for t in tails)
    ch = [_pa(t[2][j] if fuse_cls else None for t in tails) for j in range(4)]
    cin = box0.shape[1]
    wbytes = sum(64 * cin * 2 + ((80 * lv.cls.shape[1] + nc * 80) * 2 if fuse_cls else 0) for lv in levels)
    flops = sum(2.0 * B * lv.box.shape[2] * lv.box.shape[3] * (hid * 21 + 200 + 64 * cin + ((80 * lv.cls.shape[1] + nc * 80) if fuse_cls else 0)) for lv in levels)
    nbytes = sum(_nb(lv.box, lv.cls) for lv in levels) + wbytes + nb + (B * A * (4 + nc) * 4 if pred is not None else 0)
    rec = _tr("head_tail_decode_kernel", nbytes, flops, note=f"{n} levels, box tail{' + class chain' if fuse_cls else ''} + NMS keys")
    if not _try_launch(rec, "ey_head_tail_decode_levels_nms", L.lib().ey_head_tail_decode_levels_nms, L.dtype_code(box0.dtype), B, n, Hs, Ws, st, boxp, boxcs, cin, 64, bw, bb,
                       clsp, clscs, int(fuse_cls), clscin, 80, *ch, nc, *qa, hid, _p(pred), A, offs, float(conf), _p(mask), buf.data_ptr(), nb, L.stream()):
        return None
    return Candidates(buf, B, nc, A, conf, classes, pred)


def scale_img(x, ratio, flip_lr=False, gs=32):
    """scale_img(x.flip(3) if flip_lr else x, ratio, gs=gs) of the reference (utils/torch_utils.py:423-432; ratio 1 and no flip -> x itself)
    on a contiguous NCHW image batch: one kernel (flip + bilinear resize + 0.447 padding)."""
    import math
    L.require_device(x, "scale_img")
    if ratio == 1.0 and not flip_lr:
        return x
    x = x.contiguous()
    B, Cc, H, W = x.shape
    if ratio == 1.0:
        hs, ws, Hp, Wp = H, W, H, W
    else:
        hs, ws = int(H * ratio), int(W * ratio)
        Hp, Wp = (math.ceil(v * ratio / gs) * gs for v in (H, W))
    y = torch.empty((B, Cc, Hp, Wp), dtype=x.dtype, device=x.device)
    with _tr("scale_img_kernel", _nb(x, y), 8.0 * y.numel()):
        L.check(L.lib().ey_scale_img(L.dtype_code(x.dtype), B, Cc, H, W, x.data_ptr(), hs, ws, Hp, Wp, int(bool(flip_lr)), 0.447, y.data_ptr(), L.stream()), "ey_scale_img")
    return y


def tta_merge(pred, lo, hi, scale, flip, img_hw, out, out_off):
    """out[:, :, out_off : out_off + hi - lo] = _descale_pred(pred, flip, scale, img_hw)[:, :, lo:hi] (reference tasks.py:388-408)."""
    L.require_device(pred, "tta_merge")
    B, no, A = pred.shape
    if pred.dtype != torch.float32 or out.dtype != torch.float32 or not pred.is_contiguous() or not out.is_contiguous():
        raise TypeError("tta_merge: contiguous fp32 (B, no, A) tensors")
    with _tr("tta_merge_kernel", 8 * B * no * (hi - lo)):
        L.check(L.lib().ey_tta_merge(B, no, A, pred.data_ptr(), lo, hi, float(scale), int(flip or 0), int(img_hw[0]), int(img_hw[1]), out.data_ptr(), out.shape[2],
                                     out_off, L.stream()), "ey_tta_merge")
    return out


def copy_bytes(dst, src):
    """dst (device, contiguous) <- src (contiguous; device or PINNED HOST memory, which the device reads over PCIe itself) with a plain
    copy kernel in the current stream: unlike an H2D hipMemcpyAsync it runs beside kernels of other streams (engine/model.py)."""
    L.require_device(dst, "copy_bytes")
    n = dst.numel() * dst.element_size()
    if not (dst.is_contiguous() and src.is_contiguous() and src.numel() * src.element_size() == n and n % 16 == 0 and (src.is_cuda or src.is_pinned())
            and dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0):
        raise ValueError("copy_bytes: contiguous 16-byte aligned tensors of equal byte size (source on the device or in pinned host memory)")
    L.check(L.lib().ey_copy_linear(src.data_ptr(), dst.data_ptr(), n, L.stream()), "ey_copy_linear")
    return dst


def e2e_topk(pred, k, want_index=False):
    """Detect.postprocess (reference head.py:167-189): pred fp32 (B,4+nc,A) with x1y1x2y2 rows -> (B,k,6) fp32 rows
    [x1,y1,x2,y2,score,class], the k best (anchor, class) pairs per image in descending score order."""
    L.require_device(pred, "e2e_topk")
    B, no, A = _dense(pred, "e2e_topk: pred (B,4+nc,A)", torch.float32, (_ANY, _ANY, _ANY), pred.device).shape
    nc = no - 4
    if not 0 < k <= A:
        raise ValueError(f"e2e_topk: k={k} must be in 1..A={A}")
    out = torch.empty((B, k, 6), dtype=torch.float32, device=pred.device)
    index = torch.empty((B, k), dtype=torch.int32, device=pred.device) if want_index else None
    nb = L.lib().ey_e2e_topk_workspace_bytes(B, nc, A)
    ws = _workspace("e2e_topk", None, nb, pred.device)
    with _tr("e2e_topk(score+select)", pred.numel() * 4 + out.numel() * 4):
        L.check(L.lib().ey_e2e_topk(B, nc, A, pred.data_ptr(), k, out.data_ptr(), _p(index), ws.data_ptr(), nb, L.stream()), "ey_e2e_topk")
    return (out, index) if want_index else out


def nms(pred, conf_thres, iou_thres, max_det, max_nms, max_wh, agnostic, class_mask=None, multi_label=False, return_workspace=False):
    """pred fp32 (B,4+nc,A) contiguous -> (boxes (B,max_det,6) fp32, count (B,) int32, index (B,max_det) int32).
    return_workspace (tests): also the workspace tensor (keys, class ids, the fast path's per-image scratch with its n_sel / n_total / done words)."""
    L.require_device(pred, "nms")
    B, no, A = _dense(pred, "nms: pred (B,4+nc,A)", torch.float32, (_ANY, _ANY, _ANY), pred.device).shape
    dev = pred.device
    multi_label = bool(multi_label) and no - 4 > 1  # reference ops.py:240
    boxes, count, index = _nms_out(B, max_det, 6, dev)
    nbytes = L.lib().ey_nms_workspace_bytes_ml(B, no - 4, A) if multi_label else L.lib().ey_nms_workspace_bytes(B, A)
    ws = _workspace("nms", None, nbytes, dev)
    with _tr("nms(score+sort_greedy)", _nb(pred, boxes)):
        L.check(L.lib().ey_nms(B, no - 4, A, pred.data_ptr(), float(conf_thres), float(iou_thres), int(max_det), int(max_nms), float(max_wh), int(bool(agnostic)), int(bool(multi_label)),
                               _p(class_mask), boxes.data_ptr(), count.data_ptr(), index.data_ptr(),
                               ws.data_ptr(), nbytes, L.stream()), "ey_nms")
    return (boxes, count, index, ws) if return_workspace else (boxes, count, index)


def obb_decode_levels(levels, pred):
    """levels: list (<= 4) of (box, cls, angle, stride, a_off) NHWC views -> pred (B, 4+nc+1, A) fp32: DFL expectation, dist2rbox, class
    sigmoids and the angle row of the OBB head, every level in ONE launch (ey_obb_decode_levels)."""
    n = len(levels)
    box0, cls0 = levels[0][0], levels[0][1]
    L.require_device(box0, "obb_decode")
    _no_block("obb decode")
    B, nc = box0.shape[0], cls0.shape[1]
    _dense(pred, "obb_decode: pred (B, 4+nc+1, A)", torch.float32, (B, 4 + nc + 1, _ANY), box0.device)
    (Hs, Ws, st, offs), ptr, cs = _level_arrays(levels, 3, 3, 4)
    nbytes = sum(_nb(lv[0], lv[1], lv[2]) for lv in levels) + _nb(pred)
    with _tr("obb_decode_kernel", nbytes, sum(2.0 * B * lv[0].shape[2] * lv[0].shape[3] * 220 for lv in levels), note=f"{n} levels"):
        L.check(L.lib().ey_obb_decode_levels(L.dtype_code(box0.dtype), B, n, Hs, Ws, st, ptr[0], cs[0], ptr[1], cs[1], ptr[2], cs[2], nc, pred.data_ptr(), pred.shape[2],
                                             offs, L.stream()), "ey_obb_decode_levels")
    return pred


def probiou(obb1, obb2):
    """(N,5), (M,5) xywhr fp32 device tensors -> the (N,M) fp32 ProbIoU matrix (ey_probiou)."""
    L.require_device(obb1, "probiou")
    o1, o2 = obb1.float().contiguous(), obb2.float().contiguous()
    for name, o in (("obb1", o1), ("obb2", o2)):
        _dense(o, f"probiou: {name} (xywhr rows)", torch.float32, (_ANY, 5), o1.device)
    out = torch.empty((o1.shape[0], o2.shape[0]), dtype=torch.float32, device=o1.device)
    with _tr("obb_probiou_kernel", _nb(o1, o2, out), 60.0 * out.numel()):
        L.check(L.lib().ey_probiou(o1.shape[0], o2.shape[0], o1.data_ptr(), o2.data_ptr(), out.data_ptr(), L.stream()), "ey_probiou")
    return out


def nms_rotated(pred, conf_thres, iou_thres, max_det, max_nms, max_wh, agnostic, class_mask=None):
    """pred fp32 (B,4+nc+1,A) contiguous (xywh, scores, angle) -> (rows (B,max_det,7) fp32 = x,y,w,h,conf,cls,angle, count (B,) int32,
    index (B,max_det) int32): fast-NMS on ProbIoU (ey_nms_rotated), single label."""
    L.require_device(pred, "nms_rotated")
    B, no, A = _dense(pred, "nms_rotated: pred (B,4+nc+1,A)", torch.float32, (_ANY, _ANY, _ANY), pred.device).shape
    rows, count, index = _nms_out(B, max_det, 7, pred.device)
    nbytes = L.lib().ey_nms_rotated_workspace_bytes(B, A, int(max_nms))
    ws = _workspace("nms_rotated", None, nbytes, pred.device)
    with _tr("nms_rotated(init+score+rank+pair+resolve)", _nb(pred, rows), kernels=5):
        L.check(L.lib().ey_nms_rotated(B, no - 5, A, pred.data_ptr(), float(conf_thres), float(iou_thres), int(max_det), int(max_nms), float(max_wh), int(bool(agnostic)),
                                       _p(class_mask), rows.data_ptr(), count.data_ptr(), index.data_ptr(),
                                       ws.data_ptr(), nbytes, L.stream()), "ey_nms_rotated")
    return rows, count, index


def nms_rotated_ml(pred, conf_thres, iou_thres, max_det, max_nms, max_wh, agnostic, class_mask=None):
    """nms_rotated in the validation regime (ey_nms_rotated_ml): every (anchor, class) score above conf is a candidate, the max_nms best go
    through fast-NMS on ProbIoU.  Same operands and outputs as nms_rotated; index is the anchor of each row."""
    L.require_device(pred, "nms_rotated_ml")
    B, no, A = _dense(pred, "nms_rotated_ml: pred (B,4+nc+1,A)", torch.float32, (_ANY, _AtLeast(6), _ANY), pred.device).shape
    if class_mask is not None:
        _dense(class_mask, "nms_rotated_ml: class_mask", torch.uint8, (no - 5,), pred.device)
    rows, count, index = _nms_out(B, max_det, 7, pred.device)
    nbytes = L.lib().ey_nms_rotated_ml_workspace_bytes(B, no - 5, A, int(max_nms))
    ws = _workspace("nms_rotated_ml", None, nbytes, pred.device)
    with _tr("nms_rotated_ml(init+score+select+rank+pair+resolve)", _nb(pred, rows), kernels=6):
        L.check(L.lib().ey_nms_rotated_ml(B, no - 5, A, pred.data_ptr(), float(conf_thres), float(iou_thres), int(max_det), int(max_nms), float(max_wh),
                                          int(bool(agnostic)), _p(class_mask), rows.data_ptr(), count.data_ptr(), index.data_ptr(),
                                          ws.data_ptr(), nbytes, L.stream()), "ey_nms_rotated_ml")
    return rows, count, index


def probiou_batch(pred, pred_off, gt, gt_off, out_off=None, out=None):
    """ProbIoU of a batch (ey_probiou_batch): pred fp32 (N_total,5) and gt fp32 (M_total,5) xywhr rows grouped by image through the host
    lists pred_off / gt_off (B+1 entries from 0).  Image b's row-major [M_b][N_b] matrix batch_probiou(gt_b, pred_b) lands at element
    out_off[b] of the flat fp32 buffer `out` (packed one after the other by default).  -> (out, out_off)."""
    L.require_device(pred, "probiou_batch")
    _no_block("probiou_batch")
    pred_off, gt_off, out_off, sizes, end = _pair_offsets("probiou_batch", pred_off, gt_off, out_off)
    B, dev = len(out_off), pred.device
    _dense(pred, "probiou_batch: pred (N,5)", torch.float32, (_AtLeast(pred_off[-1]), 5), dev)
    _dense(gt, "probiou_batch: gt (M,5)", torch.float32, (_AtLeast(gt_off[-1]), 5), dev)
    out = _dense_out("probiou_batch: out=", out, torch.float32, (_AtLeast(end),), dev)
    with _tr("obb_probiou_batch_kernel", _nb(pred, gt) + 4 * sum(sizes), 60.0 * sum(sizes), note=f"B{B} N{pred_off[-1]} M{gt_off[-1]}"):
        L.check(L.lib().ey_probiou_batch(B, pred.data_ptr(), _ia(pred_off), gt.data_ptr(), _ia(gt_off), out.data_ptr(), _la(out_off), L.stream()), "ey_probiou_batch")
    return out, out_off


def _kpt_levels(levels, kpt_shape, what):
    """levels: list of (kpt map (B,nk,H,W) NHWC view, stride, a_off) -> the ctypes arrays both keypoint decode kernels take."""
    n = len(levels)
    m0 = levels[0][0]
    L.require_device(m0, what)
    _no_block(what)
    nkpt, ndim = int(kpt_shape[0]), int(kpt_shape[1])
    for lv in levels:
        if lv[0].dim() != 4 or lv[0].shape[1] != nkpt * ndim or lv[0].dtype != m0.dtype or lv[0].shape[0] != m0.shape[0]:
            raise ValueError(f"{what}: every level must be a (B, {nkpt * ndim}, H, W) map of one dtype, got {tuple(lv[0].shape)} {lv[0].dtype}")
    (Hs, Ws, st, offs), ptr, cs = _level_arrays(levels, 1, 1, 2)
    return (L.dtype_code(m0.dtype), m0.shape[0], n, Hs, Ws, st, ptr[0], cs[0], nkpt, ndim), offs


def kpts_decode_levels(levels, kpt_shape, out):
    """levels: list (<= 4) of (kpt logits (B,nk,H,W) NHWC view, stride, a_off); out: fp32 (B, nk, A) view whose rows are contiguous (e.g.
    pred[:, 4+nc:] of the prediction tensor) -> the decoded keypoint rows of every level in ONE launch (ey_kpts_decode_levels)."""
    head, offs = _kpt_levels(levels, kpt_shape, "kpts_decode_levels")
    B, nk = head[1], head[8] * head[9]
    if out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != B or out.shape[1] != nk or out.stride(2) != 1 or out.stride(1) != out.shape[2] or (
            B > 1 and out.stride(0) < nk * out.shape[2]):
        raise ValueError(f"kpts_decode_levels: out must be a float32 (B, {nk}, A) tensor with contiguous rows, got {tuple(out.shape)} {out.dtype} strides {out.stride()}")
    A = out.shape[2]
    with _tr("kpts_decode_levels_kernel", sum(_nb(lv[0]) for lv in levels) + 4 * B * nk * A, 3.0 * B * nk * A, note=f"{len(levels)} levels"):
        L.check(L.lib().ey_kpts_decode_levels(*head, out.data_ptr(), out.stride(0) if B > 1 else nk * A, A, offs, L.stream()), "ey_kpts_decode_levels")
    return out


def kpts_decode_rows(levels, kpt_shape, index, count, A=None, out=None):
    """The keypoints of the rows NMS kept (ey_kpts_decode_rows): levels as for kpts_decode_levels, index int32 (B,max_det) anchors, count
    int32 (B,) -> fp32 (B, max_det, nkpt, ndim) (`out`, or a new tensor); rows beyond the count or without a valid anchor are zeros.  A: the
    anchor count of the prediction (default: the end of the last level).  No host synchronisation."""
    head, offs = _kpt_levels(levels, kpt_shape, "kpts_decode_rows")
    B, nkpt, ndim = head[1], head[8], head[9]
    dev = levels[0][0].device
    _dense(index, "kpts_decode_rows: index (B, max_det)", torch.int32, (B, _AtLeast(1)), dev)
    _dense(count, "kpts_decode_rows: count", torch.int32, (B,), dev)
    if A is None:
        A = max(int(lv[2]) + lv[0].shape[2] * lv[0].shape[3] for lv in levels)
    max_det = index.shape[1]
    out = _dense_out("kpts_decode_rows: out=", out, torch.float32, (B, max_det, nkpt, ndim), dev)
    with _tr("kpts_decode_rows_kernel", _nb(index, out), 3.0 * out.numel()):
        L.check(L.lib().ey_kpts_decode_rows(*head, int(A), offs, max_det, index.data_ptr(), count.data_ptr(), out.data_ptr(), L.stream()), "ey_kpts_decode_rows")
    return out


def kpt_iou(pred, pred_off, gt, gt_off, area, sigma, out_off=None, out=None):
    """OKS of a batch (ey_kpt_iou): pred fp32 (N_total,K,ndim) and gt fp32 (M_total,K,3) grouped by image through the host lists pred_off /
    gt_off (B+1 entries from 0), area fp32 (M_total,), sigma fp32 (K,).  Image b's row-major [M_b][N_b] matrix lands at element out_off[b] of
    the flat fp32 buffer `out` (packed one after the other by default).  -> (out, out_off)."""
    L.require_device(pred, "kpt_iou")
    _no_block("kpt_iou")
    pred_off, gt_off, out_off, sizes, end = _pair_offsets("kpt_iou", pred_off, gt_off, out_off)
    B, dev = len(out_off), pred.device
    _dense(pred, "kpt_iou: pred (N,K,ndim)", torch.float32, (_AtLeast(pred_off[-1]), _ANY, _ANY), dev)
    K, ndim = int(pred.shape[1]), int(pred.shape[2])
    _dense(gt, "kpt_iou: gt (M,K,3)", torch.float32, (_AtLeast(gt_off[-1]), K, 3), dev)
    _dense(area, "kpt_iou: area", torch.float32, (_AtLeast(gt_off[-1]),), dev)
    _dense(sigma, "kpt_iou: sigma", torch.float32, (_AtLeast(K),), dev)
    out = _dense_out("kpt_iou: out=", out, torch.float32, (_AtLeast(end),), dev)
    with _tr("kpt_iou_kernel", _nb(pred, gt) + 4 * sum(sizes), 12.0 * K * sum(sizes), note=f"B{B} N{pred_off[-1]} M{gt_off[-1]} K{K}"):
        L.check(L.lib().ey_kpt_iou(B, K, ndim, pred.data_ptr(), _ia(pred_off), gt.data_ptr(), _ia(gt_off), area.data_ptr(), sigma.data_ptr(), _la(out_off),
                                   out.data_ptr(), L.stream()), "ey_kpt_iou")
    return out, out_off


def classify_pool(x, w, bias, act, out=None):
    """Classify.conv + pool + flatten (ey_classify_pool): x logical (B, C1, H, W) NHWC view, w (Cout, C1) in x's dtype (BN folded), bias fp32
    (Cout,) -> fp32 (B, Cout) = mean over the pixels of act(conv1x1(x) + bias).  The (B, Cout, H, W) map is never written."""
    x = L.as_nhwc(as_tensor(x))
    L.require_device(x, "classify_pool")
    _no_block("classify_pool")
    B, C1, H, W = x.shape
    Cout = int(_dense(w, "classify_pool: w (Cout, C1)", x.dtype, (_ANY, C1), x.device).shape[0])
    _dense(bias, "classify_pool: bias", torch.float32, (Cout,), x.device)
    out = _dense_out("classify_pool: out=", out, torch.float32, (B, Cout), x.device)
    with _tr("classify_pool_kernel", _nb(x, w, bias, out), 2.0 * B * H * W * C1 * Cout):
        L.check(L.lib().ey_classify_pool(L.dtype_code(x.dtype), B, H * W, C1, Cout, int(act), x.data_ptr(), L.cstride(x), w.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                         L.stream()), "ey_classify_pool")
    return out


def classify_linear_softmax(pooled, w, bias):
    """Classify.linear + softmax + top-k (ey_classify_linear_softmax): pooled fp32 (B, K), w (nc, K) f16 or fp32, bias fp32 (nc,) ->
    (logits (B, nc), probs (B, nc), top index int32 (B, min(nc, 5)), top probability (B, min(nc, 5))), all fp32 but the index.  Equal
    probabilities rank the lower class index first."""
    L.require_device(pooled, "classify_linear_softmax")
    _no_block("classify_linear_softmax")
    dev = pooled.device
    B, K = _dense(pooled, "classify_linear_softmax: pooled (B, K)", torch.float32, (_ANY, _ANY), dev).shape
    nc = int(_dense(w, "classify_linear_softmax: w (nc, K)", w.dtype, (_ANY, K), dev).shape[0])  # (its dtype is the entry point's to refuse)
    _dense(bias, "classify_linear_softmax: bias", torch.float32, (nc,), dev)
    k5 = min(nc, 5)
    logits = torch.empty((B, nc), dtype=torch.float32, device=dev)
    probs = torch.empty((B, nc), dtype=torch.float32, device=dev)
    topi = torch.empty((B, k5), dtype=torch.int32, device=dev)
    topp = torch.empty((B, k5), dtype=torch.float32, device=dev)
    with _tr("classify_linear_softmax_kernel", _nb(pooled, w, bias, logits, probs, topi, topp), 2.0 * B * K * nc):
        L.check(L.lib().ey_classify_linear_softmax(L.dtype_code(w.dtype), B, K, nc, pooled.data_ptr(), w.data_ptr(), bias.data_ptr(), logits.data_ptr(), probs.data_ptr(),
                                                   topi.data_ptr(), topp.data_ptr(), L.stream()), "ey_classify_linear_softmax")
    return logits, probs, topi, topp


def classify_transform(images, size, dtype, out=None, swap_rb=True):
    """classify_transforms(size) on the device (ey_classify_transform): images = contiguous uint8 (B, h, w, 3) device tensor (BGR like cv2)
    -> (B, 3, size, size) `dtype` RGB in [0, 1]: Resize(size) (Pillow's antialiased bilinear) + CenterCrop(size) + ToTensor in one launch."""
    _dense(images, "classify_transform: images (B, h, w, 3)", torch.uint8, (_ANY, _ANY, _ANY, 3), torch.device("cuda"))
    L.require_device(images, "classify_transform")
    _no_block("classify_transform")
    B, h, w, _ = images.shape
    S = int(size)
    out = _dense_out("classify_transform: out=", out, dtype, (B, 3, S, S), images.device)
    with _tr("classify_transform_kernel", _nb(images, out)):
        L.check(L.lib().ey_classify_transform(L.dtype_code(dtype), images.data_ptr(), B, h, w, 3 * w, 3 * w * h, out.data_ptr(), S, int(swap_rb), L.stream()),
                "ey_classify_transform")
    return out


def linear_assignment(costs, thresh, out=None):
    """Thresholded linear assignments of a batch in one launch (ey_linear_assignment; what lap.lapjv(cost, extend_cost=True, cost_limit=thresh)
    computes, reference trackers/utils/matching.py:20-61).  costs: a list of 2-D float32 device tensors (n_b, m_b) with unit column stride,
    sizes may differ and may be 0; thresh: one float or one per problem.  -> (row_to_col (B, nmax), col_to_row (B, mmax)) int32, -1 =
    unmatched; entries past a problem's own n_b / m_b are -1 when the tensors are made here and untouched in out= (a pair of contiguous
    int32 tensors (B, >= nmax), (B, >= mmax))."""
    costs = list(costs)
    B = len(costs)
    if B == 0:
        raise ValueError("linear_assignment: no problems")
    dev = costs[0].device
    L.require_device(costs[0], "linear_assignment")
    _no_block("linear_assignment")
    for c in costs:
        if not torch.is_tensor(c) or c.dim() != 2 or c.dtype != torch.float32 or c.device != dev or (c.numel() > 0 and ((c.shape[1] > 1 and c.stride(1) != 1) or (c.shape[0] > 1 and c.stride(0) < c.shape[1]))):
            raise ValueError("linear_assignment: every cost matrix must be a 2-D float32 tensor with unit column stride on one device")
    th = [float(thresh)] * B if not isinstance(thresh, (list, tuple)) else [float(t) for t in thresh]
    if len(th) != B:
        raise ValueError(f"linear_assignment: {len(th)} thresholds for {B} problems")
    nmax, mmax = max(int(c.shape[0]) for c in costs), max(int(c.shape[1]) for c in costs)
    if out is None:
        r2c, c2r = (_dense_out("linear_assignment: out=", None, torch.int32, (B, max(n, 1)), dev, fill=-1) for n in (nmax, mmax))
    else:
        r2c, c2r = (_dense(t, f"linear_assignment: out= {name}", torch.int32, (B, _AtLeast(n)), dev) for t, name, n in ((out[0], "row_to_col", nmax), (out[1], "col_to_row", mmax)))
    desc = torch.tensor([[c.data_ptr(), c.shape[0], c.shape[1], c.stride(0) if c.shape[0] > 1 and c.numel() else max(int(c.shape[1]), 1)] for c in costs], dtype=torch.int64).to(dev)
    tht = torch.tensor(th, dtype=torch.float32).to(dev)
    nb = int(L.lib().ey_linear_assignment_workspace_bytes(B, nmax, mmax))
    ws = _workspace("linear_assignment", None, nb, dev)
    with _tr("linear_assignment_kernel", _nb(*costs, r2c, c2r), note=f"{B} x <= {nmax}x{mmax}"):
        L.check(L.lib().ey_linear_assignment(B, desc.data_ptr(), tht.data_ptr(), nmax, mmax, r2c.data_ptr(), int(r2c.shape[1]), c2r.data_ptr(), int(c2r.shape[1]),
                                             ws.data_ptr(), nb, L.stream()), "ey_linear_assignment")
    return r2c, c2r


def bytetrack_state(streams, max_tracks, device):
    """the device state ey_bytetrack_update advances: all zero = fresh trackers."""
    B, T = int(streams), int(max_tracks)
    return {"kf": torch.zeros((B, T, 72), dtype=torch.float64, device=device), "slot_i": torch.zeros((B, T, 8), dtype=torch.int32, device=device),
            "slot_f": torch.zeros((B, T, 2), dtype=torch.float32, device=device), "hdr": torch.zeros((B, 4), dtype=torch.int32, device=device)}


def bytetrack_update(rows, count, state, settings, out=None, workspace=None):
    """One ByteTrack frame for B streams in one launch (ey_bytetrack_update).  rows float32 (B, cap, 6) x1,y1,x2,y2,score,cls; count int32 (B,);
    state: the dict of bytetrack_state(), advanced in place; settings: track_high_thresh, track_low_thresh, new_track_thresh, match_thresh,
    track_buffer, fuse_score.  -> (out_rows float32 (B, cap, 8) = x1,y1,x2,y2,id,score,cls,idx, ids int32 (B, cap), counts int32 (B,)); only
    the first counts[b] rows of stream b are written.  out=: that triple, to write instead."""
    L.require_device(rows, "bytetrack_update")
    _no_block("bytetrack_update")
    dev = rows.device
    B, cap = (int(v) for v in _dense(rows, "bytetrack_update: rows (B, cap, 6)", torch.float32, (_ANY, _AtLeast(1), 6), dev).shape[:2])
    _dense(count, "bytetrack_update: count", torch.int32, (B,), dev)
    T = int(state["kf"].shape[1])
    for k, (shape, dt) in {"kf": ((B, T, 72), torch.float64), "slot_i": ((B, T, 8), torch.int32), "slot_f": ((B, T, 2), torch.float32), "hdr": ((B, 4), torch.int32)}.items():
        _dense(state[k], f"bytetrack_update: state['{k}']", dt, shape, dev)
    if out is not None and (len(out := tuple(out)) != 3 or any(t is None for t in out)):
        raise ValueError("bytetrack_update: out= must be the (out_rows, ids, counts) tensors")
    out = tuple(_dense_out(f"bytetrack_update: out= {name}", out and out[i], dt, shape, dev, fill=0)
                for i, (name, shape, dt) in enumerate((("out_rows", (B, cap, 8), torch.float32), ("ids", (B, cap), torch.int32), ("counts", (B,), torch.int32))))
    workspace = _workspace("bytetrack_update", workspace, int(L.lib().ey_bytetrack_workspace_bytes(B, cap, T)), dev)
    s = settings
    with _tr("bytetrack_update_kernel", _nb(rows, *out), note=f"{B} streams x {cap} rows, {T} slots"):
        L.check(L.lib().ey_bytetrack_update(B, cap, T, float(s["track_high_thresh"]), float(s["track_low_thresh"]), float(s["new_track_thresh"]), float(s["match_thresh"]),
                                            int(30 / 30.0 * s["track_buffer"]), int(bool(s["fuse_score"])), rows.data_ptr(), count.data_ptr(), state["kf"].data_ptr(),
                                            state["slot_i"].data_ptr(), state["slot_f"].data_ptr(), state["hdr"].data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                            out[2].data_ptr(), workspace.data_ptr(), workspace.numel(), L.stream()), "ey_bytetrack_update")
    return out


def mask_contours_launch(masks, windows, contour_cap, vertex_cap, out=None):
    """One ey_mask_contours launch: masks uint8 (n >= 1, h, w), windows int32 (n, 4) or None -> (lens int32 (n, contour_cap), verts int32
    (n, vertex_cap, 2), info int32 (n, 4) = contours found, vertices found, flags, 0), see include/edgeyolo_hip.h.  out=: that triple, to
    write instead."""
    n, h, w = (int(v) for v in masks.shape)
    dev = masks.device
    if out is not None and (len(out := tuple(out)) != 3 or any(t is None for t in out)):
        raise ValueError("mask_contours: out= must be the (lens, verts, info) tensors")
    out = tuple(_dense_out(f"mask_contours: out= {name}", out and out[i], torch.int32, shape, dev)
                for i, (name, shape) in enumerate((("lens", (n, contour_cap)), ("verts", (n, vertex_cap, 2)), ("info", (n, 4)))))
    nb = int(L.lib().ey_mask_contours_workspace_bytes(n, h, w))
    ws = _workspace("mask_contours", None, nb, dev)
    with _tr("mask_contours_kernel", _nb(masks, *out), note=f"{n} masks {h}x{w}, room for {contour_cap} contours / {vertex_cap} vertices each"):
        L.check(L.lib().ey_mask_contours(n, h, w, masks.data_ptr(), _p(windows), contour_cap, vertex_cap,
                                         out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), nb, L.stream()), "ey_mask_contours")
    return out


def mask_contours(masks, boxes=None, out=None, _contour_capacity=64, _vertex_capacity=4096):
    """External contours of binary masks on the device (ey_mask_contours: what cv2.findContours(m, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)[0]
    gives per mask).  masks: contiguous uint8 or bool (n, h, w) device tensor, non-zero = set, left untouched.  boxes: optional
    (n, >= 4) xyxy in mask pixels, the boxes process_mask cropped the masks to: mask i is scanned inside floor / ceil of box i only (every
    set pixel must lie inside it; the result is then the same).  -> a list of n lists of (k, 2) int32 numpy arrays of x, y, in OpenCV's
    order (last found first).  Only the counts and the vertices cross to the host.  The launch writes into fixed-size buffers; when a mask
    needs more room than they have, they grow to what the kernel counted and the launch is repeated, so nothing is ever cut short.
    out=: the (lens, verts, info) tensors of mask_contours_launch for the first launch."""
    _dense(masks, "mask_contours: masks (n, h, w)", (torch.uint8, torch.bool), (_ANY, _ANY, _ANY), None)
    L.require_device(masks, "mask_contours")
    _no_block("mask_contours")
    n, h, w = (int(v) for v in masks.shape)
    if h < 1 or w < 1:
        raise ValueError(f"mask_contours: masks of {h} x {w} pixels")
    dev = masks.device
    windows = None
    if boxes is not None:
        if not torch.is_tensor(boxes) or boxes.dim() != 2 or boxes.shape[0] != n or boxes.shape[1] < 4 or boxes.device != dev:
            raise ValueError(f"mask_contours: boxes must be a ({n}, >= 4) xyxy tensor on {dev}")
        b = torch.nan_to_num(boxes[:, :4].float(), nan=0.0).clamp(0, max(h, w))
        windows = torch.cat([b[:, :2].floor(), b[:, 2:].ceil()], 1).to(torch.int32).contiguous()
    if n == 0:
        return []
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    import numpy as np
    ccap, vcap = max(int(_contour_capacity), 1), max(int(_vertex_capacity), 1)
    if out is not None:  # (their sizes are the first launch's capacities)
        out = tuple(out)
        if len(out) != 3 or not all(torch.is_tensor(t) for t in out) or out[0].dim() != 2 or out[1].dim() != 3 or out[0].shape[1] < 1 or out[1].shape[1] < 1:
            raise ValueError("mask_contours: out= must be the (lens, verts, info) tensors of mask_contours_launch")
        ccap, vcap = int(out[0].shape[1]), int(out[1].shape[1])
    for attempt in range(2):  # the second launch has the room the first one asked for
        lens, verts, info = mask_contours_launch(masks, windows, ccap, vcap, out if attempt == 0 else None)
        counts = info.cpu().numpy()
        if (counts[:, 2] & 2).any():
            raise L.HipLibraryError(f"mask_contours: a border walk passed its step bound in mask {int(np.nonzero(counts[:, 2] & 2)[0][0])}")
        if int(counts[:, 0].max()) <= ccap and int(counts[:, 1].max()) <= vcap:
            break
        ccap, vcap = max(ccap, int(counts[:, 0].max())), max(vcap, int(counts[:, 1].max()))
    else:
        raise L.HipLibraryError("mask_contours: the second launch asked for more room than the first one counted")
    nc, nv = info[:, 0:1], info[:, 1:2]
    lens = lens[torch.arange(ccap, device=dev)[None, :] < nc].cpu().numpy()
    verts = verts[torch.arange(vcap, device=dev)[None, :] < nv].cpu().numpy()
    ends = np.cumsum(lens)
    res, k = [], 0
    for i in range(n):
        c = int(counts[i, 0])
        res.append([verts[ends[j] - lens[j]:ends[j]] for j in range(k + c - 1, k - 1, -1)])
        k += c
    return res


MATCH_MAX_T = 16  # mtc::MAX_T: the most IoU thresholds ey_match_batch takes


def match_batch(rows, count, gt_cls, gt_off, iouv, nc, gt=None, xform=None, iou=None, iou_off=None, iou_n=None, cm_conf=0.25, cm_iou=0.45, tp=None,
                matrix=None):
    """Validation matching of a batch in one launch (ey_match_batch, include/edgeyolo_hip.h).  rows fp32 (B, max_det, >= 6) x1,y1,x2,y2,conf,cls
    (a channel window of a wider row buffer is fine) and count int32 (B,), as nms_device returns them; gt fp32 (M, 4) xyxy, gt_cls int32 (M,)
    device tensors grouped by image through the host list gt_off (B+1 entries from 0); xform fp32 (B, 5) padx, pady, gain, w0, h0 or None.
    iou / iou_off / iou_n: matrix mode, the flat [gt x pred] buffer and the host offsets a pair-matrix op returned plus the images' kept counts
    as the host knows them (the matrices' row lengths), in the place of the boxes.
    iouv: host sequence of 1..16 thresholds.  tp: uint8 (B, max_det, T) to fill below each image's count, or None for no true positives;
    matrix: int32 ((nc+1)^2,) to add to, or None for no confusion matrix.  -> (tp, matrix) as given."""
    L.require_device(rows, "match_batch")
    _no_block("match_batch")
    dev = rows.device
    if rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] < 6 or rows.shape[1] < 1 or rows.stride(2) != 1 or rows.stride(1) < rows.shape[2] or (
            rows.shape[0] > 1 and rows.stride(0) != rows.shape[1] * rows.stride(1)):
        raise ValueError(f"match_batch: rows must be a float32 (B, max_det, >= 6) tensor whose rows are dense windows of one buffer, got {tuple(rows.shape)} "
                         f"{rows.dtype} strides {rows.stride()}")
    B, max_det, stride = int(rows.shape[0]), int(rows.shape[1]), int(rows.stride(1))
    _dense(count, "match_batch: count", torch.int32, (B,), dev)
    gt_off = [int(v) for v in gt_off]
    if len(gt_off) != B + 1 or gt_off[0] != 0 or any(b < a for a, b in zip(gt_off, gt_off[1:])):
        raise ValueError("match_batch: gt_off must have B+1 non-decreasing entries starting at 0")
    M = gt_off[-1]
    thr = [float(v) for v in iouv]
    T = len(thr)
    if not 1 <= T <= MATCH_MAX_T:
        raise ValueError(f"match_batch: {T} thresholds (1..{MATCH_MAX_T} are built)")
    _dense(gt_cls, "match_batch: gt_cls", torch.int32, (_AtLeast(M),), dev)
    if iou is None:
        _dense(gt, "match_batch: gt (M,4)", torch.float32, (_AtLeast(M), 4), dev)
        if xform is not None:
            _dense(xform, "match_batch: xform (B,5)", torch.float32, (B, 5), dev)
        off = None
    else:
        if iou_off is None or len(iou_off) != B or iou_n is None or len(iou_n) != B:
            raise ValueError("match_batch: matrix mode needs iou_off and iou_n with B entries")
        off, ld = [int(v) for v in iou_off], [int(v) for v in iou_n]
        if any(n < 0 or n > max_det for n in ld) or any(o < 0 for b, o in enumerate(off) if gt_off[b + 1] > gt_off[b]):
            raise ValueError(f"match_batch: iou_n must lie in [0, {max_det}] and iou_off must not be negative where the image has labels")
        need = max([off[b] + (gt_off[b + 1] - gt_off[b]) * ld[b] for b in range(B) if gt_off[b + 1] > gt_off[b]] + [0])
        _dense(iou, "match_batch: iou", torch.float32, (_AtLeast(need),), dev)
        xform = None
    if tp is not None:
        _dense(tp, "match_batch: tp=", torch.uint8, (B, max_det, T), dev)
    if matrix is not None:
        _dense(matrix, "match_batch: matrix=", torch.int32, ((int(nc) + 1) ** 2,), dev)
    with _tr("match_batch_kernel", 24 * B * max_det + 20 * M + (B * max_det * T if tp is not None else 0), 12.0 * max_det * M, note=f"B{B} max_det{max_det} M{M} T{T}"):
        L.check(L.lib().ey_match_batch(B, max_det, stride, rows.data_ptr(), count.data_ptr(), _p(xform), _p(gt) if iou is None else None, gt_cls.data_ptr(),
                                       _ia(gt_off), _p(iou), None if off is None else _la(off), None if off is None else _ia(ld), T, _fa(thr), int(nc), float(cm_conf), float(cm_iou),
                                       _p(tp), _p(matrix), L.stream()), "ey_match_batch")
    return tp, matrix
