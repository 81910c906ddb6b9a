"""Composite blocks of the detection path, HIP-backed.  Constructor signatures, attribute names and state_dict
keys follow the reference's ultralytics/nn/modules/block.py (line numbers cited per class).  chunk/split/cat
never copy: producers write straight into channel slices of one NHWC buffer (`out=`), residual adds ride in the
conv epilogue (`res=`).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F  # pack time only: softplus/tanh on 4+1 scalar parameters, the text projection of a vocabulary

from .conv import Conv, DSConv, DWConv, GhostConv, RepConv, _Packed, _act_code, fold_bn
from .. import _ops as ops
from ... import _lib as L

__all__ = ("DFL", "Proto", "SPPF", "C2f", "C2fAttn", "MaxSigmoidAttnBlock", "BNContrastiveHead","C3", "C3k", "C3k2", "Bottleneck", "Attention", "PSABlock", "C2PSA", "LinearAttention",
           "PSABlock_LinearAttention", "C2PSA_LinearAttention", "AAttn", "ABlock", "A2C2f", "DSBottleneck", "DSC3k", "DSC3K2_Wavelet",
           "DSC3K2", "Mlp", "CMlp", "LocalAgg", "GlobalSparseAttn", "SelfAttn", "LGLBlock", "DSC3K2_LGL",
           "AdaHyperedgeGen", "AdaHGConv", "AdaHGComputation", "C3AH", "FuseModule", "HyperACE", "DownsampleConv", "FullPAD_Tunnel",
           "RepBottleneck", "RepCSP", "RepNCSPELAN4", "ELAN1", "AConv", "ADown", "SPPELAN", "CBLinear", "CBFuse", "SCDown", "RepVGGDW", "CIB", "C2fCIB", "PSA",
           "C2", "GhostBottleneck", "C3Ghost", "SPP", "ResNetBlock", "ResNetLayer")


def _slot(buf, i, c):
    return buf[:, i * c:(i + 1) * c]


def _stacked(*convs):
    """1x1 convs over the same input as one launch: their (BN-folded) filters and biases concatenated along Cout."""
    ws, bs = zip(*(m.folded() for m in convs))
    return torch.cat(ws, 0), torch.cat(bs, 0)


def _stacked_act(*convs):
    """The one activation code a stacked launch of these convs would apply, or None when they do not share one."""
    acts = {_act_code(m.act) for m in convs}
    return acts.pop() if len(acts) == 1 else None


def _repeated(conv):
    """conv(a + p) == conv over the virtual concat [a | p] with the weight repeated along Cin: one launch, no add kernel."""
    w, b = conv.folded()
    return torch.cat((w, w), 1), b


def _scale_vec(mod, tag, param, x):
    """Device fp32 (C,) scale vector for ops.scale_add_channels on x: a 0-d, (1,) or (C,) `param` rounded to x's dtype (as the reference's
    product is) and broadcast over the channels; cached on `mod` (a _Packed)."""
    C = x.shape[1]
    return mod._packed((tag, x.dtype, x.device, C), lambda: param.detach().to(x.dtype).float().expand(C).to(x.device).contiguous())


def _pool_pyramid(cv_in, cv_out, x, out):
    """cv_in -> three chained 5x5 max-pools (ONE ey_sppf_pool launch into slots 1-3 of a 4 c buffer) -> cv_out over the 4-way concat."""
    x = L.as_nhwc(x)
    B, _, H, W = x.shape
    c = cv_in.conv.out_channels
    buf = L.empty_nhwc(B, 4 * c, H, W, x.dtype, x.device)
    cv_in(x, out=buf[:, :c])
    ops.sppf_pool(_slot(buf, 0, c), _slot(buf, 1, c), _slot(buf, 2, c), _slot(buf, 3, c))
    return cv_out(buf, out=out)


def _attn_ffn(attn, ffn, x, out=None):
    """x + attn(x); x + ffn(x): both residual adds ride in conv epilogues."""
    x = attn(x, res=x)
    return ffn[1](ffn[0](x), out=out, res=x)


def _c2psa(mod, x, out):
    """cv1 splits into (a, b); the blocks of `mod.m` chain on b, the last writing back into b's half of cv1's buffer; cv2 reads the buffer."""
    t = mod.cv1(x)
    b = t[:, mod.c:]
    for i, m in enumerate(mod.m):
        b = m(b, out=t[:, mod.c:] if i == len(mod.m) - 1 else None)
    return mod.cv2(t, out=out)


def _ds_pair(cv1, cv2, x, add, out):
    """[x +] cv2(cv1(x)) of two DSConvs: both and the residual as one band kernel on the small maps, else two launches."""
    y = ops.dsb_pair(cv1, cv2, x, add, out=out)
    if y is not None:
        return y
    return cv2(cv1(x), out=out, res=x if add else None)


class _Chains(_Packed):
    """Mixin: pointwise chains of a block -- runs of 1x1 convs whose pixels do not interact -- as ONE launch each (nn/_block.py tiled
    programs: recorded from the ordinary module code below; one 512-thread workgroup per 64-pixel tile with register-resident weights
    where ey_block_fast_plan takes the chain, else one 256-thread workgroup per 32-pixel tile walks the stages).  The caches
    hold packed weights, so they live in _Packed's cache and drop with it.  `pw_chains = False` keeps one launch per conv."""

    # True, False, or a tuple of chain names.  Measured on MI355X inside the benchmarked step (batch 32, C2PSA at 256 channels, 20x20,
    # kernel trace; profiles/chain_fast_*): the four-conv tail as one launch 22.9 us on the register-weight executor (44.5 us on
    # block_tile_kernel).  The two-conv head as one launch takes 23.9 us against 10.8 + 15.2 us for its two conv_pwn launches: the
    # step is not faster for it in the pipelined mode (see profiles/chain_fast_bench_parent_vs_branch.txt), so it stays off
    pw_chains = ("proj_ffn_cv2",)

    def _chain(self, name):
        from .._block import BlockCache
        return self._packed(("chain", name), lambda: BlockCache(f"{type(self).__name__}.{name}", tiled=True))

    def _chains_on(self, x, name=None):
        on = self.pw_chains if isinstance(self.pw_chains, bool) else (name is None or name in self.pw_chains)
        return bool(on) and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float16 and ops.RECORD is None


class DFL(nn.Module):
    """Integral of the distribution-focal-loss bins (reference block.py:72-90).  Parameter holder: the expectation is
    computed inside the fused head-decode kernel with the fixed weights 0..c1-1."""

    def __init__(self, c1=16):
        super().__init__()
        self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
        self.conv.weight.data[:] = torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1)
        self.c1 = c1


class Proto(_Packed):
    """Mask prototypes of the Segment head (reference block.py:112-129): cv3(cv2(upsample(cv1(x)))).  `upsample` is an nn.ConvTranspose2d kept
    as the parameter holder; it runs as ONE GEMM launch with a scatter epilogue (ey_deconv2x2)."""

    def __init__(self, c1, c_=256, c2=32):
        super().__init__()
        self.cv1 = Conv(c1, c_, k=3)
        self.upsample = nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True)
        self.cv2 = Conv(c_, c_, k=3)
        self.cv3 = Conv(c_, c2)

    def forward(self, x, out=None):
        return self.cv3(self.cv2(ops.deconv2x2(self, self.cv1(x), self.upsample)), out=out)


class Bottleneck(nn.Module):
    """reference block.py:467-480."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2

    def forward(self, x, out=None):
        return self.cv2(self.cv1(x), out=out, res=x if self.add else None)


class C2f(nn.Module):
    """reference block.py:357-379."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    def forward(self, x, out=None):
        B, _, H, W = x.shape  # x may be a VirtualCat (upsample+concat folded into cv1)
        c, n = self.c, len(self.m)
        buf = L.empty_nhwc(B, self.cv2.conv.in_channels, H, W, x.dtype, x.device)  # (2 + n) slots, and those a subclass's cv2 reads beyond them
        self.cv1(x, out=buf[:, :2 * c])
        for i, m in enumerate(self.m):
            m(_slot(buf, 1 + i, c), out=_slot(buf, 2 + i, c))
        self._extra_slots(buf, c, n)
        return self.cv2(buf, out=out)

    def _extra_slots(self, buf, c, n):
        """Hook: a subclass fills the slots behind the n blocks' (C2fAttn)."""


class C3(_Packed):
    """reference block.py:382-396."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0) for _ in range(n)))

    def _cv12(self):
        """cv1 and cv2 are both 1x1 convs over the same input: stack their (BN-folded) filters -> one launch."""
        return _stacked(self.cv1, self.cv2)

    def _cv12_act(self):
        """The one activation code of the stacked launch: cv1 and cv2 carry the same activation (the model's: SiLU, or the YAML's `activation:`)."""
        act = _stacked_act(self.cv1, self.cv2)
        if act is None:
            raise NotImplementedError("C3: cv1 and cv2 with different activations cannot share the stacked launch")
        return act

    def forward(self, x, out=None, cv12=None):
        """cv12 (extension): the stacked cv1|cv2 output when the caller has already computed it (chained into the producer of x)."""
        x = L.as_nhwc(x)
        B, _, H, W = x.shape
        c_ = self.cv1.conv.out_channels
        # buf = [cv1(x) -> m(.) in place | cv2(x)]: the bottleneck chain rewrites slot 0 in place (its last conv reads a
        # temporary and adds slot 0 pixel-by-pixel as the residual), so cat() never happens
        buf = cv12 if cv12 is not None else ops.conv2d(self, [x], self._cv12, 1, 1, 0, self._cv12_act(), tag="cv12")
        slot, t, spare = buf[:, :c_], buf[:, :c_], None
        for m in self.m:
            if isinstance(m, DSBottleneck):
                # a DSBottleneck may run as ONE band kernel whose workgroups read halo rows of their neighbours' input: never in place.
                # The chain alternates between slot 0 and a spare buffer (n = 2: slot 0 -> spare -> slot 0)
                if t.data_ptr() == slot.data_ptr():
                    if spare is None:
                        spare = L.empty_nhwc(B, c_, H, W, x.dtype, x.device)
                    t = m(t, out=spare)
                else:
                    t = m(t, out=slot)
            else:
                t = m(t, out=slot)
        if t.data_ptr() != slot.data_ptr():  # odd DSBottleneck count: the chain ended in the spare buffer -> cv3 reads [spare | cv2(x)] as a virtual concat
            return ops.conv2d(self.cv3, [t, buf[:, c_:]], self.cv3.folded, 1, 1, 0, _act_code(self.cv3.act), out=out)
        return self.cv3(buf, out=out)


class C3k(C3):
    """reference block.py:868-876."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, k=3):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=(k, k), e=1.0) for _ in range(n)))


class C3k2(C2f):
    """reference block.py:857-865."""

    def __init__(self, c1, c2, n=1, c3k=False, e=0.5, g=1, shortcut=True):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(C3k(self.c, self.c, 2, shortcut, g) if c3k else Bottleneck(self.c, self.c, shortcut, g) for _ in range(n))


class MaxSigmoidAttnBlock(_Packed):
    """Max-sigmoid attention of YOLO-World (reference block.py:544-576): x = proj_conv(x) gated per pixel and head by
    sigmoid(max_n(embed . gl(text)) / sqrt(hc) + bias) * scale.  The projected guide gl(text) is constant for a vocabulary: it is computed
    once (torch, fp32, rounded once to the storage type) and cached per (vocabulary, dtype, device); the gate is ONE launch
    (ey_max_sigmoid_attn).  The module holds its text (`set_text`); the graph executor never passes it.  Built: no embed conv (c1 == ec,
    which the parse rule gives every C2fAttn of the worldv2 YAML) and head width hc = 32."""

    def __init__(self, c1, c2, nh=1, ec=128, gc=512, scale=False):
        super().__init__()
        self.nh = nh
        self.hc = c2 // nh
        if c1 != ec:
            raise NotImplementedError(f"MaxSigmoidAttnBlock: c1={c1} != ec={ec} needs the embed conv `ec`, which is not built (the worldv2 YAML never has one)")
        if self.hc != 32 or self.hc * nh != c2:
            raise NotImplementedError(f"MaxSigmoidAttnBlock: c2={c2} with nh={nh} gives head width hc={c2 / nh:g}; the kernel is built for hc=32")
        if ec != c2:
            raise ValueError(f"MaxSigmoidAttnBlock: ec={ec} must equal nh * hc = {c2}")
        self.ec = None
        self.gl = nn.Linear(gc, ec)
        self.bias = nn.Parameter(torch.zeros(nh))
        self.proj_conv = Conv(c1, c2, k=3, s=1, act=False)
        self.scale = nn.Parameter(torch.ones(1, nh, 1, 1)) if scale else 1.0
        self.__dict__["_txt"] = None

    def set_text(self, txt):
        """txt: (Bg, n, gc) text embeddings (any device / float dtype), Bg = 1 or the batch size; drops the cached guide."""
        self.__dict__["_txt"] = txt
        self._cache = {}

    def guide(self, dtype, device):
        """(Bg, n, nh * hc) projected text in `dtype` on `device`, cached until the text or the parameters change."""
        txt = self.__dict__.get("_txt")
        if txt is None:
            raise RuntimeError("MaxSigmoidAttnBlock: no text set (WorldModel.set_classes / set_text supply it)")
        if not 1 <= txt.shape[1] <= L.MSA_MAX_TEXTS:
            raise NotImplementedError(f"MaxSigmoidAttnBlock: {txt.shape[1]} texts; the kernel takes 1 to {L.MSA_MAX_TEXTS}")

        def build():
            w, b = self.gl.weight.detach().to(device).float(), self.gl.bias.detach().to(device).float()
            g = F.linear(txt.detach().to(device).float(), w, b).to(dtype).contiguous()
            sc = self.scale.detach().to(device).float().flatten().contiguous() if torch.is_tensor(self.scale) else None
            return g, self.bias.detach().to(device).float().contiguous(), sc

        return self._packed(("guide", dtype, device), build)

    def forward(self, x, out=None):
        x = L.as_nhwc(x)
        g, bias, sc = self.guide(x.dtype, x.device)
        if g.shape[0] not in (1, x.shape[0]):
            raise ValueError(f"MaxSigmoidAttnBlock: text for {g.shape[0]} images, batch of {x.shape[0]}")
        return ops.max_sigmoid_attn(x, self.proj_conv(x), g, bias, sc, self.nh, out=out)


class C2fAttn(C2f):
    """C2f with a max-sigmoid attention branch on its last hidden map (reference block.py:579-596): one more slot in the concat buffer,
    (3 + n) c channels.  cv1 writes the first two slots, each Bottleneck its own, proj_conv a scratch map, ey_max_sigmoid_attn the last slot;
    cv2 reads the buffer."""

    def __init__(self, c1, c2, n=1, ec=128, nh=1, gc=512, shortcut=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.cv2 = Conv((3 + n) * self.c, c2, 1)
        self.attn = MaxSigmoidAttnBlock(self.c, self.c, gc=gc, ec=ec, nh=nh)

    def _extra_slots(self, buf, c, n):
        self.attn(_slot(buf, 1 + n, c), out=_slot(buf, 2 + n, c))


class BNContrastiveHead(nn.Module):
    """Region-text similarity head of WorldDetect (reference block.py:670-692): exp(logit_scale) * <BatchNorm(x), normalize(w)> + bias.
    Parameter holder: for a fixed vocabulary the whole expression is affine in the class tower's hidden map and WorldDetect folds it into
    the tower's closing 1x1 conv."""

    def __init__(self, embed_dims):
        super().__init__()
        self.norm = nn.BatchNorm2d(embed_dims)
        self.bias = nn.Parameter(torch.tensor([-10.0]))
        self.logit_scale = nn.Parameter(-1.0 * torch.ones([]))


class SPPF(nn.Module):
    """reference block.py:204-223: cv1 -> three chained 5x5 max-pools -> cv2 over the 4-way concat."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        if k != 5:
            raise NotImplementedError("SPPF pooling kernel is built for k=5 (the only value the YAMLs use)")
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)

    def forward(self, x, out=None):
        return _pool_pyramid(self.cv1, self.cv2, x, out)


class SPP(nn.Module):
    """Spatial pyramid pooling of YOLOv3-SPP (reference block.py:186-201): cv2(cat(y, m5(y), m9(y), m13(y))), y = cv1(x).  A 5x5 max-pool
    applied twice is the 9x9 pool and applied three times the 13x13 one (stride 1, -inf padding), so k = (5, 9, 13) runs on the SPPF chain kernel
    (ey_sppf_pool) bit for bit; no other k is built.  `m` keeps the reference's pooling modules (no parameters; never called)."""

    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        if tuple(k) != (5, 9, 13):
            raise NotImplementedError(f"SPP: k={tuple(k)}; the pooling kernel is built for k=(5, 9, 13), the chain of three 5x5 pools")
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * (len(k) + 1), c2, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])

    def forward(self, x, out=None):
        return _pool_pyramid(self.cv1, self.cv2, x, out)


# ----------------------------------------------------------------------------------------------- attention
class Attention(_Packed):
    """Softmax self-attention of the YOLO11 baseline (reference block.py:1000-1053)."""

    def __init__(self, dim, num_heads=8, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim ** -0.5
        nh_kd = self.key_dim * num_heads
        h = dim + nh_kd * 2
        self.qkv = Conv(dim, h, 1, act=False)
        self.proj = Conv(dim, dim, 1, act=False)
        self.pe = Conv(dim, dim, 3, 1, g=dim, act=False)

    def forward(self, x, out=None, res=None):
        x = L.as_nhwc(x)
        B, C, H, W = x.shape
        nh, kd, hd = self.num_heads, self.key_dim, self.head_dim
        qkv = self.qkv(x)
        a = ops.softmax_attention(qkv, nh, kd, hd, self.scale)
        per = 2 * kd + hd
        v = L.empty_nhwc(B, C, H, W, x.dtype, x.device)
        for h in range(nh):  # v.reshape(B, C, H, W): gather the per-head value channels
            ops.copy_slice(qkv[:, h * per + 2 * kd:(h + 1) * per], v[:, h * hd:(h + 1) * hd])
        p = self.pe(v)
        return ops.conv2d(self, [a, p], lambda: _repeated(self.proj), 1, 1, 0, L.ACT_NONE, out=out, res=res, tag="proj2")  # proj(a + p)


class PSABlock(nn.Module):
    """x + Attention(x); x + FFN(x) (reference block.py:3376-3408)."""

    def __init__(self, c, attn_ratio=0.5, num_heads=None, mlp_ratio=2.0, qkv_bias=True, proj_bias=False, **kwargs):
        super().__init__()
        heads = max(1, (c // 64) if num_heads is None else int(num_heads))
        assert c % heads == 0, f"PSABlock: channels {c} must be divisible by num_heads {heads}"
        self.attn = Attention(c, num_heads=heads, attn_ratio=attn_ratio)
        hidden = int(c * mlp_ratio)
        self.ffn = nn.Sequential(Conv(c, hidden, k=1, s=1, act=True), Conv(hidden, c, k=1, s=1, act=False))

    def forward(self, x, out=None):
        return _attn_ffn(self.attn, self.ffn, x, out)


class C2PSA(nn.Module):
    """reference block.py:1100-1139."""

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.m = nn.Sequential(*(PSABlock(self.c, attn_ratio=0.5, num_heads=self.c // 64) for _ in range(n)))

    def forward(self, x, out=None):
        return _c2psa(self, x, out)


class LinearAttention(_Packed):
    """reference block.py:3348-3373: qkv 1x1 (bias) -> k softmax over head_dim, q softmax over N -> ctx = k^T v ->
    y = q ctx -> proj 1x1.  Extra kwargs are swallowed like the reference's **kwargs."""

    def __init__(self, dim, num_heads, attn_ratio=None, qkv_bias=False, proj_bias=True, **kwargs):
        super().__init__()
        assert dim % num_heads == 0, "LinearAttention: dim must be divisible by num_heads"
        self.dim = dim
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.qkv = nn.Conv2d(dim, 3 * dim, kernel_size=1, bias=qkv_bias)
        self.proj = nn.Conv2d(dim, dim, kernel_size=1, bias=proj_bias)

    def _qkv_folded(self):
        return fold_bn(self.qkv.weight, self.qkv.bias, None)

    def _proj_folded(self):
        """(w, b) of proj in fp32; without a bias b is None (the launch then adds none), not zeros."""
        return self.proj.weight.detach().float(), self.proj.bias.detach().float() if self.proj.bias is not None else None

    def forward(self, x, out=None, res=None):
        qkv = ops.conv2d(self, [x], self._qkv_folded, 1, 1, 0, L.ACT_NONE, tag="qkv")
        y = ops.linear_attention(qkv, self.num_heads)
        return ops.conv2d(self, [y], self._proj_folded, 1, 1, 0, L.ACT_NONE, out=out, res=res, tag="proj")


class PSABlock_LinearAttention(nn.Module):
    """reference block.py:3412-3449."""

    def __init__(self, dim, attn_ratio=0.5, num_heads=None, mlp_ratio=2.0, qkv_bias=True, proj_bias=False, fmap="elu", eps=1e-6):
        super().__init__()
        self.attn = LinearAttention(dim=dim, num_heads=num_heads, attn_ratio=attn_ratio, qkv_bias=qkv_bias, proj_bias=proj_bias, fmap=fmap, eps=eps)
        hidden = int(dim * mlp_ratio)
        self.ffn = nn.Sequential(Conv(dim, hidden, k=1, s=1, act=True), Conv(hidden, dim, k=1, s=1, act=False))

    def forward(self, x, out=None):
        return _attn_ffn(self.attn, self.ffn, x, out)


class C2PSA_LinearAttention(_Chains):
    """reference block.py:3452-3497.  f16: 7 launches -> 3: [cv1 -> qkv] | linear attention | [proj(+x) -> ffn -> ffn(+x) -> cv2]."""

    def __init__(self, c1, c2, n=1, e=0.5, attn_ratio=0.5, num_heads=None, mlp_ratio=2.0, fmap="elu"):
        super().__init__()
        assert c1 == c2, "C2PSA_LinearAttention requires c1 == c2"
        self.c = int(c1 * e)
        heads = max(1, (self.c // 64) if num_heads is None else num_heads)
        assert self.c % heads == 0
        self.cv1 = Conv(c1, 2 * self.c, k=1, s=1)
        self.m = nn.Sequential(*[PSABlock_LinearAttention(dim=self.c, attn_ratio=attn_ratio, num_heads=heads, mlp_ratio=mlp_ratio, fmap=fmap)
                                 for _ in range(n)])
        self.cv2 = Conv(2 * self.c, c1, k=1, s=1)

    def forward(self, x, out=None):
        if len(self.m) == 1 and self._chains_on(x):
            y = self._forward_chained(x, out)
            if y is not None:
                return y
        return _c2psa(self, x, out)

    def _forward_chained(self, x, out):
        blk, c = self.m[0], self.c
        at = blk.attn

        def head(x0):  # cv1 -> qkv of the attention branch
            t = self.cv1(x0)
            return [t, ops.conv2d(at, [t[:, c:]], at._qkv_folded, 1, 1, 0, L.ACT_NONE, tag="qkv")]

        def tail(y, t):  # x1 = b + proj(y); x2 = x1 + ffn(x1) (written over b, in place per pixel); cv2([a | x2])
            b = t[:, c:]
            x1 = ops.conv2d(at, [y], at._proj_folded, 1, 1, 0, L.ACT_NONE, res=b, tag="proj")
            blk.ffn[1](blk.ffn[0](x1), out=b, res=x1)
            return [self.cv2(t, out=out)]

        got = self._chain("cv1_qkv").run(head, [L.as_nhwc(x)]) if self._chains_on(x, "cv1_qkv") else None
        t, qkv = got if got is not None else head(L.as_nhwc(x))
        y = ops.linear_attention(qkv, at.num_heads)
        res = self._chain("proj_ffn_cv2").run(tail, [y, t], [out] if out is not None else None) if self._chains_on(x, "proj_ffn_cv2") else None
        if res is None:  # (not block-executable: the same tail, one launch per conv)
            return tail(y, t)[0]
        return res[0]


# ----------------------------------------------------------------------------------------------- area attention (YOLOv12)
class AAttn(_Packed):
    """Area attention (reference block.py:1272-1356): y = proj(attn(q, k, v) + pe(v)).  qk holds [q: heads*32 | k: heads*32]; the H*W
    tokens are cut into `area` contiguous row-major runs attended separately (ey_area_attention).  qk and v run as one stacked 1x1 conv,
    and proj reads the virtual concat [attn | pe(v)] with its weight repeated (one launch, no add kernel)."""

    def __init__(self, dim, num_heads, area=1):
        super().__init__()
        self.area = area
        self.num_heads = num_heads
        self.head_dim = head_dim = dim // num_heads
        all_head_dim = head_dim * self.num_heads
        self.qk = Conv(dim, all_head_dim * 2, 1, act=False)
        self.v = Conv(dim, all_head_dim, 1, act=False)
        self.proj = Conv(all_head_dim, dim, 1, act=False)
        self.pe = Conv(all_head_dim, dim, 5, 1, 2, g=dim, act=False)

    def forward(self, x, out=None, res=None):
        B, _, H, W = x.shape
        if (H * W) % self.area:  # the reference's reshape to (B*area, N/area, C) fails here too
            raise ValueError(f"AAttn: {H}x{W} = {H * W} tokens do not split into {self.area} equal areas")
        x = L.as_nhwc(x)
        c = self.num_heads * self.head_dim
        qkv = ops.conv2d(self, [x], lambda: _stacked(self.qk, self.v), 1, 1, 0, L.ACT_NONE, tag="qkv")  # [q | k | v]
        v = qkv[:, 2 * c:]
        p = self.pe(v)
        a = ops.area_attention(qkv[:, :c], qkv[:, c:2 * c], v, self.num_heads, self.area, self.head_dim ** -0.5)
        return ops.conv2d(self, [a, p], lambda: _repeated(self.proj), 1, 1, 0, L.ACT_NONE, out=out, res=res, tag="proj2")


class ABlock(_Packed):
    """x + AAttn(x); x + mlp(x) (reference block.py:1359-1406)."""

    def __init__(self, dim, num_heads, mlp_ratio=1.2, area=1):
        super().__init__()
        self.attn = AAttn(dim, num_heads=num_heads, area=area)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(Conv(dim, mlp_hidden_dim, 1), Conv(mlp_hidden_dim, dim, 1, act=False))
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Conv2d):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)

    def forward(self, x, out=None):
        x = self.attn(x, res=x)
        h = self.mlp[0](x)
        if h.shape[1] % 8 == 0:
            return self.mlp[1](h, out=out, res=x)
        # a hidden width off the MFMA conv's 8-channel granularity (the default mlp_ratio 1.2 at 64 channels; the YAMLs use 2.0 / 1.5)
        # takes the direct conv, which has no residual epilogue: the add is the layer-scale kernel with gamma = 1 (exact)
        return ops.scale_add_channels(x, _scale_vec(self, "ones", torch.ones(()), x), self.mlp[1](h), out=out)


class A2C2f(_Packed):
    """R-ELAN (reference block.py:1409-1465): cv1 -> n x (2 ABlocks | C3k) chained -> cv2 over the concat of all of them, written
    straight into slices of one buffer; with a2 and residual, x + gamma * cv2(...) as one per-channel HIP launch."""

    def __init__(self, c1, c2, n=1, a2=True, area=1, residual=False, mlp_ratio=2.0, e=0.5, g=1, shortcut=True):
        super().__init__()
        c_ = int(c2 * e)
        assert c_ % 32 == 0, "Dimension of ABlock be a multiple of 32."
        num_heads = c_ // 32
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv((1 + n) * c_, c2, 1)
        init_values = 0.01
        self.gamma = nn.Parameter(init_values * torch.ones((c2)), requires_grad=True) if a2 and residual else None
        self.m = nn.ModuleList(
            nn.Sequential(*(ABlock(c_, num_heads, mlp_ratio, area) for _ in range(2))) if a2 else C3k(c_, c_, 2, shortcut, g) for _ in range(n))

    def forward(self, x, out=None):
        B, _, H, W = x.shape  # x may be a VirtualCat (upsample+concat folded into cv1)
        c, n = self.cv1.conv.out_channels, len(self.m)
        buf = L.empty_nhwc(B, (1 + n) * c, H, W, x.dtype, x.device)
        self.cv1(x, out=buf[:, :c])
        for i, m in enumerate(self.m):
            src, dst = _slot(buf, i, c), _slot(buf, 1 + i, c)
            if isinstance(m, nn.Sequential):
                for j, blk in enumerate(m):
                    src = blk(src, out=dst if j == len(m) - 1 else None)
            else:
                m(src, out=dst)
        if self.gamma is None:
            return self.cv2(buf, out=out)
        x = ops.as_tensor(x)
        return ops.scale_add_channels(x, _scale_vec(self, "gamma", self.gamma, x), self.cv2(buf), out=out)


# ----------------------------------------------------------------------------------------------- DS / wavelet
class DSBottleneck(nn.Module):
    """reference block.py:1467-1503."""

    def __init__(self, c1, c2, shortcut=True, e=0.5, k1=3, k2=5, d2=1):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = DSConv(c1, c_, k1, s=1, p=None, d=1)
        self.cv2 = DSConv(c_, c2, k2, s=1, p=None, d=d2)
        self.add = shortcut and c1 == c2

    def forward(self, x, out=None):
        return _ds_pair(self.cv1, self.cv2, x, self.add, out)


class DSC3k(C3):
    """reference block.py:1506-1562."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, k1=3, k2=5, d2=1):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(DSBottleneck(c_, c_, shortcut=shortcut, e=1.0, k1=k1, k2=k2, d2=d2) for _ in range(n)))


_FILTERS = None
_HAAR = (0.7071067811865476, 0.7071067811865476), (-0.7071067811865476, 0.7071067811865476)  # pywt.Wavelet("haar").dec_lo / dec_hi


def wavelet_filters():
    """{name: (dec_lo, dec_hi)} of every discrete PyWavelets wavelet with at most 64 taps, and {name: length} of the longer ones
    (nn/wavelet_filters.json, recorded from pywt.Wavelet(name); the package does not need pywt)."""
    global _FILTERS
    if _FILTERS is None:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wavelet_filters.json")) as f:
            d = json.load(f)
        _FILTERS = ({k: (tuple(v["dec_lo"]), tuple(v["dec_hi"])) for k, v in d["filters"].items()}, dict(d["too_long"]))
    return _FILTERS


class _PywtDWT2D(_Packed):
    """Single-level 2-D analysis with a pywt filter bank (reference block.py:3582-3642): reflect padding by k/2 - 1, then a depthwise
    k x k conv with stride 2 over the outer products of h0 = dec_lo[::-1] and h1 = dec_hi[::-1] (fp32, cast to the activation dtype).
    A bank equal to Haar's (haar, db1, ...) runs the dedicated 2x2 kernel; every other bank runs ey_dwt.  `mode` is stored and ignored,
    as in the reference (always reflect)."""

    def __init__(self, wave="haar", mode="symmetric"):
        super().__init__()
        table, too_long = wavelet_filters()
        if wave in too_long:
            raise NotImplementedError(f"wavelet '{wave}': {too_long[wave]} taps; filter banks longer than 64 taps are not built")
        if wave not in table:
            raise NotImplementedError(f"wavelet '{wave}': not a discrete PyWavelets wavelet (pywt.wavelist(kind='discrete') names them)")
        self.wave_name, self.mode = wave, mode
        lo, hi = table[wave]
        self.k = len(lo)
        self.pad = self.k // 2 - 1  # (every discrete pywt bank has even length)
        self.haar = (lo, hi) == _HAAR
        h0 = torch.tensor(lo[::-1], dtype=torch.float32)
        h1 = torch.tensor(hi[::-1], dtype=torch.float32)
        e = lambda a, b: torch.einsum("i,j->ij", a, b)  # noqa: E731  (fp32 products, rounded once: block.py:3604-3607)
        self.taps32 = torch.stack([e(h0, h0), e(h0, h1), e(h1, h0), e(h1, h1)])  # (4,k,k) CPU constant, not module state

    def taps(self, x):
        """Device fp32 taps with the values the reference convolves with in x's dtype (self.weight.to(dtype=x.dtype))."""
        return self._packed(("taps", x.dtype, x.device), lambda: self.taps32.to(x.dtype).float().to(x.device).contiguous())

    def check_size(self, H, W):
        if H < 2 or W < 2:
            raise ValueError(f"_PywtDWT2D: feature map {H}x{W} is too small for a 2x2 Haar step" if self.haar else
                             f"_PywtDWT2D: feature map {H}x{W} is too small")
        if self.pad >= H or self.pad >= W:  # F.pad(mode="reflect") refuses these in the reference
            raise ValueError(f"_PywtDWT2D('{self.wave_name}'): reflect padding {self.pad} needs a feature map larger than {H}x{W}")

    def subbands(self, x):
        """(B,C,H,W) -> (B,4C,H/2,W/2) with channel blocks LL|LH|HL|HH."""
        self.check_size(x.shape[2], x.shape[3])
        x = L.as_nhwc(x)
        return ops.dwt_haar(x) if self.haar else ops.dwt(x, self.taps(x), self.k)

    def forward(self, x):
        y = self.subbands(x)
        c = x.shape[1]
        return y[:, :c], y[:, c:2 * c], y[:, 2 * c:3 * c], y[:, 3 * c:]


class _WaveletEnhancer(_Packed):
    """reference block.py:3645-3710:  b + tanh(gamma) * fuse(cat[b, w0 up(f_ll LL), w1 up(f_h LH), w2 up(f_h HL), w3 up(f_h HH)]).

    A 1x1 conv commutes with bilinear upsampling, so the 3c-channel concat never exists:
        fuse(cat[...]) = SiLU( W_b b + up2x( sum_i w_i W_i P_i ) + bias ),
    i.e. a half-resolution 1x1 conv Z over the four processed sub-bands P (2c -> c, sub-band weights w_i and the BN
    scale folded into its weights) whose bilinear x2 upsample is added before the activation in the epilogue of the
    full-resolution 1x1 conv over b, which also applies tanh(gamma) and the residual b."""

    fused_z = True  # f16: the half-resolution branch as one kernel (ey_wavelet_z); False = dwt + 4-group conv + 1x1 conv (three launches)

    def __init__(self, c, use_ds=False, alpha0=(0.5, 0.2, 0.2, 0.1), wave="haar", mode="symmetric"):
        super().__init__()
        self.c = c
        self.dwt = _PywtDWT2D(wave=wave, mode=mode)
        self.f_ll = Conv(c, c // 2, k=1, s=1)
        self.f_h = (DSConv if use_ds else Conv)(c, c // 2, k=3, s=1)
        self.fuse = Conv(3 * c, c, k=1, s=1)
        self.alpha = nn.Parameter(torch.tensor(alpha0, dtype=torch.float32))
        self.gamma = nn.Parameter(torch.tensor(0.0))

    def _band_weights(self):
        w = F.softplus(self.alpha.detach().float())
        return w / (w.sum() + 1e-6)  # block.py:3697-3698

    def _subband_sets(self):
        wl, bl = self.f_ll.folded()
        if isinstance(self.f_h, DSConv):  # use_ds: the pointwise 1x1 of f_h (BN folded), also written as a centre-tap 3x3
            wp, bh = self.f_h._pw_folded()
            wh = torch.zeros(wp.shape[0], wp.shape[1], 3, 3, dtype=wp.dtype, device=wp.device)
            wh[:, :, 1:2, 1:2] = wp
        else:
            wh, bh = self.f_h.folded()
        w3 = torch.zeros_like(wh)
        w3[:, :, 1:2, 1:2] = wl  # 1x1 == 3x3 with only the centre tap (pad 1)
        return (w3, bl), (wh, bh)

    def _fuse_b(self):
        w, b = self.fuse.folded()
        return w[:, :self.c].contiguous(), b

    def _fuse_z(self):
        w, _ = self.fuse.folded()
        bw = self._band_weights().to(w.device)
        h = self.c // 2
        wz = w[:, self.c:].clone()
        for i in range(4):
            wz[:, i * h:(i + 1) * h] *= bw[i]
        return wz.contiguous(), None

    def forward(self, b, out=None, then=None):
        """then (extension): dict(mod=, folded_fn=, act=, tag=) of a 1x1 conv that reads this module's output -- where the shapes allow both run as
        one launch (ops.conv_pw_pair) and (y, y_then) is returned; y_then is None when the caller has to run that conv itself."""
        b = L.as_nhwc(b)
        B, c, H, W = b.shape
        self.dwt.check_size(H, W)
        use_ds = isinstance(self.f_h, DSConv)
        h = c // 2
        g = self._packed("tanh_gamma", lambda: float(torch.tanh(self.gamma.detach().float())))  # host scalar, cached (graph capture)
        if self.fused_z:  # f16: DWT + the four sub-band convs + Z in ONE kernel, only Z touches HBM
            Z = ops.wavelet_z(self, b, self._subband_sets, self._fuse_z, dwt=self.dwt, dw_fn=(lambda: self.f_h._dw_folded()[0]) if use_ds else None)
            if Z is not None:
                if then is not None:
                    return ops.conv_pw_pair(dict(mod=self, srcs=[b], folded_fn=self._fuse_b, act=L.ACT_SILU, out=out, res=b, addz=Z, out_scale=g, tag="b"), then)
                return ops.conv2d(self, [b], self._fuse_b, 1, 1, 0, L.ACT_SILU, out=out, res=b, addz=Z, out_scale=g, tag="b")
        sub = self.dwt.subbands(b)  # (B,4c,H/2,W/2): LL|LH|HL|HH
        P = L.empty_nhwc(B, 2 * c, H // 2, W // 2, b.dtype, b.device)
        if use_ds:  # f_ll (1x1) on LL, then the shared DSConv f_h on each high band: channel-offset views of `sub` into slices of `P`
            self.f_ll(sub[:, :c], out=P[:, :h])
            for i in (1, 2, 3):
                self.f_h(sub[:, i * c:(i + 1) * c], out=P[:, i * h:(i + 1) * h])
            return self._tail(b, P, g, out, then)
        # ONE launch for the four sub-band convs: group 0 = f_ll (a 1x1 conv written as a centre-tap 3x3) on LL, groups 1-3 =
        # the shared f_h on LH, HL, HH (weight set min(g, 1)); the groups are channel-offset slices of `sub` and `P`
        ops.conv2d(self, [sub[:, :c]], self._subband_sets, 3, 1, 1, L.ACT_SILU, out=P[:, :h], ngroup=4, src_gstride=c, y_gstride=h, w_sets=2,
                   tag="sub")
        return self._tail(b, P, g, out, then)

    def _tail(self, b, P, g, out, then):
        Z = ops.conv2d(self, [P], self._fuse_z, 1, 1, 0, L.ACT_NONE, tag="z")
        y = ops.conv2d(self, [b], self._fuse_b, 1, 1, 0, L.ACT_SILU, out=out, res=b, addz=Z, out_scale=g, tag="b")
        return (y, None) if then is not None else y


class DSC3K2_Wavelet(nn.Module):
    """reference block.py:3749-3788: cv1 -> chunk(a, b) -> b = wave(b) -> n x (DSC3k | DSBottleneck) -> cat -> cv2."""

    def __init__(self, c1, c2, n=1, dsc3k=False, e=0.5, g=1, shortcut=True, k1=3, k2=7, d2=1, **kwargs):
        super().__init__()
        use_ds = bool(kwargs.get("use_ds", False))
        wave = kwargs.get("wave", "haar")
        mode = kwargs.get("mode", "symmetric")
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1, 1)
        if dsc3k:
            self.m = nn.ModuleList(DSC3k(self.c, self.c, n=2, shortcut=shortcut, g=g) for _ in range(n))
        else:
            self.m = nn.ModuleList(DSBottleneck(self.c, self.c, shortcut=shortcut, e=1.0, k1=k1, k2=k2, d2=d2) for _ in range(n))
        self.wave = _WaveletEnhancer(self.c, use_ds=use_ds, wave=wave, mode=mode)

    def forward(self, x, out=None, tail=None):
        """tail (extension): the stride-2 3x3 Conv module that consumes this block's output and nothing else does -- cv2 and that conv then
        run as one kernel where the shape allows (ops.pw_conv3s2), and the TAIL's output is returned."""
        B, _, H, W = x.shape  # x may be a VirtualCat (upsample+concat folded into cv1)
        c, n = self.c, len(self.m)
        t = self.cv1(x)  # [a | b]
        buf = L.empty_nhwc(B, (1 + n) * c, H, W, x.dtype, x.device)  # [wave(b) | m_0 | ...]
        kw = {}
        if n and isinstance(self.m[0], C3):  # the DSC3k behind the enhancer starts with a 1x1 over the enhancer's output: chained into its tail conv
            kw["cv12"] = self.wave(t[:, c:], out=_slot(buf, 0, c), then=dict(mod=self.m[0], folded_fn=self.m[0]._cv12, act=self.m[0]._cv12_act(), tag="cv12"))[1]
        else:
            self.wave(t[:, c:], out=_slot(buf, 0, c))
        for i, m in enumerate(self.m):
            m(_slot(buf, i, c), out=_slot(buf, 1 + i, c), **kw)
            kw = {}
        # cat(a, wave(b), m...) is never built: cv2 reads the two buffers as one virtual concat
        if tail is not None:
            y = ops.pw_conv3s2(self.cv2, tail, [t[:, :c], buf])
            return y if y is not None else tail(ops.conv2d(self.cv2, [t[:, :c], buf], self.cv2.folded, 1, 1, 0, _act_code(self.cv2.act)))
        return ops.conv2d(self.cv2, [t[:, :c], buf], self.cv2.folded, 1, 1, 0, _act_code(self.cv2.act), out=out)


# ----------------------------------------------------------------------------------------------- YOLOv13: HyperACE / FullPAD
class DSC3K2(C2f):
    """reference block.py:1564-1638: C2f whose blocks are DSC3k(c, c, n=2, e=1.0) (dsc3k) or DSBottleneck(c, c, e=1.0, k1, k2, d2)."""

    def __init__(self, c1, c2, n=1, dsc3k=False, e=0.5, g=1, shortcut=True, k1=3, k2=7, d2=1):
        super().__init__(c1, c2, n, shortcut, g, e)
        if dsc3k:
            self.m = nn.ModuleList(DSC3k(self.c, self.c, n=2, shortcut=shortcut, g=g, e=1.0, k1=k1, k2=k2, d2=d2) for _ in range(n))
        else:
            self.m = nn.ModuleList(DSBottleneck(self.c, self.c, shortcut=shortcut, e=1.0, k1=k1, k2=k2, d2=d2) for _ in range(n))



# ----------------------------------------------------------------------------------------------- YOLOv13-LGL: Local-Global-Local block
def _linear_folded(lin):
    """nn.Linear on the channels of each pixel = a 1x1 conv: (w (out, in, 1, 1), b) in fp32."""
    w = lin.weight.detach().float()
    return w.view(*w.shape, 1, 1), (lin.bias.detach().float() if lin.bias is not None else torch.zeros(w.shape[0], device=w.device))


class Mlp(_Packed):
    """Token MLP fc2(GELU(fc1(x))) (reference block.py:3042-3058) on the channels of each pixel of an NHWC map: two 1x1 convs on the MFMA
    conv with the exact-erf GELU kernel between them; `res` rides in fc2's epilogue.  drop is an inference no-op."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        if act_layer is not nn.GELU:
            raise NotImplementedError("Mlp: only the exact GELU has a kernel")
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x, out=None, res=None):
        h = ops.conv2d(self, [x], lambda: _linear_folded(self.fc1), 1, 1, 0, L.ACT_NONE, tag="fc1")
        ops.gelu(h, out=h)
        return ops.conv2d(self, [h], lambda: _linear_folded(self.fc2), 1, 1, 0, L.ACT_NONE, out=out, res=res, tag="fc2")


class CMlp(_Packed):
    """Conv2d(c, rc, 3, groups=c) -> GELU -> Conv2d(rc, c, 3, groups=c) (reference block.py:3060-3076): no channel mixing, so one
    per-channel stencil kernel (ey_cmlp) with the r hidden maps in registers.  `bn`: a BatchNorm2d applied to the input inside the kernel
    (zero padding after it, as the reference pads); `gate`: return x + x * (sigmoid(.) - 1/2)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        if act_layer is not nn.GELU:
            raise NotImplementedError("CMlp: only the exact GELU has a kernel")
        self.fc1 = nn.Conv2d(in_features, hidden_features, 3, padding=1, groups=in_features)
        self.act = act_layer()
        self.fc2 = nn.Conv2d(hidden_features, out_features, 3, padding=1, groups=in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x, out=None, bn=None, gate=False):
        return ops.cmlp(self, x, self.fc1, self.fc2, bn=bn, gate=gate, out=out)


class LocalAgg(_Packed):
    """reference block.py:3078-3096, three gated steps x <- x + x * (sigmoid(f(x)) - 1/2): f = dw9 (gate in the depthwise kernel's
    epilogue); f = conv2(dw9(conv1(BN1(x)))) (BN1 folded into conv1, exact in front of a 1x1; the gate as its own launch); f = CMlp(BN2(x))
    (one kernel, BN2 applied inside because the zero padding comes after it).  drop / drop_path are inference no-ops."""

    def __init__(self, dim, mlp_ratio=4.0, drop=0.0, drop_path=0.0, act_layer=nn.GELU):
        super().__init__()
        self.pos_embed = nn.Conv2d(dim, dim, 9, padding=4, groups=dim)
        self.norm1 = nn.BatchNorm2d(dim)
        self.conv1 = nn.Conv2d(dim, dim, 1)
        self.conv2 = nn.Conv2d(dim, dim, 1)
        self.attn = nn.Conv2d(dim, dim, 9, padding=4, groups=dim)
        self.drop_path = nn.Identity()
        self.norm2 = nn.BatchNorm2d(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = CMlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        self.sg = nn.Sigmoid()

    def _conv1(self):
        bn = self.norm1
        w, b = self.conv1.weight.detach().float(), self.conv1.bias.detach().float()
        s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        sh = bn.bias.detach().float() - bn.running_mean.detach().float() * s
        return w * s.view(1, -1, 1, 1), b + w.flatten(1) @ sh

    def forward(self, x, out=None):
        x = ops.dwconv_gate(self, x, self.pos_embed, L.DWG_GATE, tag="pos")
        t = ops.conv2d(self, [x], self._conv1, 1, 1, 0, L.ACT_NONE, tag="conv1")
        t = ops.dwconv_gate(self, t, self.attn, L.DWG_PLAIN, tag="attn")
        g = ops.conv2d(self, [t], lambda: fold_bn(self.conv2.weight, self.conv2.bias, None), 1, 1, 0, L.ACT_NONE, tag="conv2")
        x = ops.sigmoid_gate(x, g, out=g)
        return self.mlp(x, out=out, bn=self.norm2, gate=True)


class GlobalSparseAttn(_Packed):
    """reference block.py:3098-3170: softmax attention over the tokens of the sr-pooled map, un-pooled by a depthwise transposed conv.
    Here: [LayerNorm + ceil-mode 2x2 average pool] (one kernel, `norm` = the caller's LayerNorm) -> qkv 1x1 conv -> ey_flash_attention over
    all Hs*Ws tokens -> [un-pool + (odd maps) bilinear resize + LayerNorm] (one kernel) -> proj 1x1 conv (+ `res`).  sr_ratio 1 or 2.
    x: an NHWC (B,C,H,W) map, or the reference's tokens (B,H*W,C) with H and W."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0.0, proj_drop=0.0, sr_ratio=1):
        super().__init__()
        self.num_heads = int(num_heads)
        head_dim = dim // self.num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.sr = int(sr_ratio)
        if self.sr > 2:
            raise NotImplementedError("GlobalSparseAttn: sr_ratio 1 and 2 have kernels (the YAMLs use 2)")
        if self.sr > 1:
            self.sampler = nn.AvgPool2d(kernel_size=self.sr, stride=self.sr, ceil_mode=True)
            self.LocalProp = nn.ConvTranspose2d(dim, dim, kernel_size=self.sr, stride=self.sr, groups=dim, bias=False)
            self.norm = nn.LayerNorm(dim)
        else:
            self.sampler = nn.Identity()
            self.LocalProp = nn.Identity()
            self.norm = nn.Identity()

    def forward(self, x, H=None, W=None, norm=None, out=None, res=None):
        if x.dim() == 3:  # (B, N, C) contiguous tokens == an NHWC (B,C,H,W) map
            B, N, C = x.shape
            if N != H * W:
                raise ValueError(f"input tokens {N} != H*W {H * W}")
            y = self.forward(x.contiguous().view(B, H, W, C).permute(0, 3, 1, 2), norm=norm)
            return y.permute(0, 2, 3, 1).reshape(B, N, C)
        x = L.as_nhwc(x)
        B, C, H, W = x.shape
        if C % self.num_heads:
            raise ValueError(f"GlobalSparseAttn: {C} channels do not split into {self.num_heads} heads")
        if self.sr > 1:
            if norm is None:  # the ceil-mode pool only exists fused behind a LayerNorm (SelfAttn.norm1)
                raise NotImplementedError("GlobalSparseAttn with sr_ratio 2 pools inside the LayerNorm kernel: pass norm=")
            t = ops.layernorm_channels(self, x, norm, pool=True, tag="pre")
        else:
            t = ops.layernorm_channels(self, x, norm, tag="pre") if norm is not None else x
        qkv = ops.conv2d(self, [t], lambda: _linear_folded(self.qkv), 1, 1, 0, L.ACT_NONE, tag="qkv")  # [q | k | v]
        a = ops.flash_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], self.num_heads, self.scale)
        if self.sr > 1:
            a = ops.unpool2_layernorm(self, a, self.LocalProp, self.norm, H, W)
        return ops.conv2d(self, [a], lambda: _linear_folded(self.proj), 1, 1, 0, L.ACT_NONE, out=out, res=res, tag="proj")


class SelfAttn(_Packed):
    """reference block.py:3172-3196: x + dw3(x); x + attn(norm1(x)); x + mlp(norm2(x)) -- the token reshapes are free in NHWC, both
    residual adds ride in the 1x1 convs' epilogues, norm1 runs inside the attention's pooling kernel."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm, sr_ratio=1):
        super().__init__()
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("SelfAttn: only nn.LayerNorm has a kernel")
        self.pos_embed = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)
        self.norm1 = norm_layer(dim)
        self.attn = GlobalSparseAttn(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop, sr_ratio=sr_ratio)
        self.drop_path = nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)

    def forward(self, x, out=None):
        x = ops.dwconv_gate(self, x, self.pos_embed, L.DWG_RESIDUAL, tag="pos")
        x = self.attn(x, norm=self.norm1, res=x)
        return self.mlp(ops.layernorm_channels(self, x, self.norm2, tag="n2"), out=out, res=x)


class LGLBlock(nn.Module):
    """reference block.py:3198-3210: LocalAgg (only with sr_ratio > 1) then SelfAttn."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm, sr_ratio=1):
        super().__init__()
        self.LocalAgg = LocalAgg(dim, mlp_ratio, drop, drop_path, act_layer) if sr_ratio > 1 else nn.Identity()
        self.SelfAttn = SelfAttn(dim, num_heads, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop, drop_path, act_layer, norm_layer, sr_ratio)

    def forward(self, x, out=None):
        return self.SelfAttn(self.LocalAgg(x), out=out)


class _DSUnit(nn.Module):
    """reference block.py:3213-3228: [x +] DSConv_k2(DSConv_k1(x)), the arithmetic of DSBottleneck(c, c, e=1) under the keys ds1 / ds2."""

    def __init__(self, c, k1=3, k2=7, d2=1, shortcut=True):
        super().__init__()
        self.ds1 = DSConv(c, c, k=k1, s=1, d=1, bias=False)
        self.ds2 = DSConv(c, c, k=k2, s=1, d=d2, bias=False)
        self.add = bool(shortcut)

    def forward(self, x, out=None):
        return _ds_pair(self.ds1, self.ds2, x, self.add, out)


class _LGLAdapter(_Packed):
    """reference block.py:3230-3273: x + gamma * LGLBlock(x), gamma a (1,) parameter (0 at initialisation) broadcast over the channels by
    ey_scale_add_channels.  heads = max(1, c // 64), moved to the nearest divisor of c."""

    def __init__(self, c, num_heads=None, sr_ratio=2, mlp_ratio=4.0, drop=0.0, attn_drop=0.0):
        super().__init__()
        if num_heads is None:
            num_heads = max(1, c // 64)
        if c % num_heads != 0:
            num_heads = min((d for d in range(1, c + 1) if c % d == 0), key=lambda d: abs(d - num_heads))
        self.lgl = LGLBlock(dim=c, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=True, qk_scale=None, drop=drop, attn_drop=attn_drop,
                            drop_path=0.0, sr_ratio=sr_ratio)
        self.gamma = nn.Parameter(torch.zeros(1))

    def forward(self, x, out=None):
        x = L.as_nhwc(x)
        return ops.scale_add_channels(x, _scale_vec(self, "gamma", self.gamma, x), self.lgl(x), out=out)


class _DSUnitWithLGL(nn.Module):
    """reference block.py:3276-3290: y = DSUnit(x); y + gamma * LGL(y)."""

    def __init__(self, c, k1, k2, d2, shortcut, lgl_heads, lgl_sr, lgl_mlp, lgl_drop, lgl_attn_drop):
        super().__init__()
        self.core = _DSUnit(c, k1=k1, k2=k2, d2=d2, shortcut=shortcut)
        self.lgl = _LGLAdapter(c, num_heads=lgl_heads, sr_ratio=lgl_sr, mlp_ratio=lgl_mlp, drop=lgl_drop, attn_drop=lgl_attn_drop)

    def forward(self, x, out=None):
        return self.lgl(self.core(x), out=out)


class DSC3K2_LGL(C2f):
    """reference block.py:3293-3345: C2f whose n blocks are _DSUnitWithLGL(c); dsc3k and g are accepted and ignored as there."""

    def __init__(self, c1, c2, n=1, dsc3k=False, e=0.5, g=1, shortcut=True, k1=3, k2=7, d2=1, lgl_heads=None, lgl_sr_ratio=2, lgl_mlp_ratio=4.0,
                 lgl_drop=0.0, lgl_attn_drop=0.0, **kwargs):
        assert e > 0, "e must be > 0"
        super().__init__(c1, c2, n, shortcut, g, e)
        self.c1, self.c2 = c1, c2
        self.m = nn.ModuleList(_DSUnitWithLGL(c=self.c, k1=k1, k2=k2, d2=d2, shortcut=shortcut, lgl_heads=lgl_heads, lgl_sr=lgl_sr_ratio,
                                              lgl_mlp=lgl_mlp_ratio, lgl_drop=lgl_drop, lgl_attn_drop=lgl_attn_drop) for _ in range(n))


class AdaHyperedgeGen(nn.Module):
    """reference block.py:1640-1716: parameter holder.  The participation matrix A is computed inside ey_hypergraph_conv (AdaHGConv)."""

    def __init__(self, node_dim, num_hyperedges, num_heads=4, dropout=0.1, context="both"):
        super().__init__()
        self.num_heads = num_heads
        self.num_hyperedges = num_hyperedges
        self.head_dim = node_dim // num_heads
        self.context = context
        self.prototype_base = nn.Parameter(torch.Tensor(num_hyperedges, node_dim))
        nn.init.xavier_uniform_(self.prototype_base)
        if context in ("mean", "max"):
            self.context_net = nn.Linear(node_dim, num_hyperedges * node_dim)
        elif context == "both":
            self.context_net = nn.Linear(2 * node_dim, num_hyperedges * node_dim)
        else:
            raise ValueError(f"Unsupported context '{context}'. Expected one of: 'mean', 'max', 'both'.")
        self.pre_head_proj = nn.Linear(node_dim, node_dim)
        self.dropout = nn.Dropout(dropout)  # identity in eval
        self.scaling = math.sqrt(self.head_dim)

    def forward(self, X):
        raise NotImplementedError("AdaHyperedgeGen runs inside AdaHGConv (ey_hypergraph_conv); A is never materialised")


class AdaHGConv(_Packed):
    """reference block.py:1719-1774: Y = GELU(node_proj(A . GELU(edge_proj(A^T X)))) + X, A = softmax over all tokens of the hyperedge
    logits -- one ey_hypergraph_conv call (five launches).  X: (B,D,H,W) NHWC (a token per pixel) or the reference's (B,N,D)."""

    def __init__(self, embed_dim, num_hyperedges=16, num_heads=4, dropout=0.1, context="both"):
        super().__init__()
        self.edge_generator = AdaHyperedgeGen(embed_dim, num_hyperedges, num_heads, dropout, context)
        self.edge_proj = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.GELU())
        self.node_proj = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.GELU())

    def forward(self, X, out=None):
        if torch.is_tensor(X) and X.dim() == 3:  # (B,N,D) contiguous == an NHWC (B,D,1,N) map
            y = ops.hypergraph_conv(self, X.permute(0, 2, 1).unsqueeze(2))
            return y.squeeze(2).permute(0, 2, 1)
        return ops.hypergraph_conv(self, X, out=out)


class AdaHGComputation(nn.Module):
    """reference block.py:1777-1815: the (B,C,H,W) <-> tokens reshapes are free in NHWC."""

    def __init__(self, embed_dim, num_hyperedges=16, num_heads=8, dropout=0.1, context="both"):
        super().__init__()
        self.embed_dim = embed_dim
        self.hgnn = AdaHGConv(embed_dim=embed_dim, num_hyperedges=num_hyperedges, num_heads=num_heads, dropout=dropout, context=context)

    def forward(self, x, out=None):
        return self.hgnn(x, out=out)


class C3AH(_Packed):
    """reference block.py:1818-1851: cv3(cat(m(cv1(x)), cv2(x))).  cv1 | cv2 run as one stacked 1x1 conv and cv3 reads the two halves as
    a virtual concat."""

    def __init__(self, c1, c2, e=1.0, num_hyperedges=8, context="both"):
        super().__init__()
        c_ = int(c2 * e)
        assert c_ % 16 == 0, "Dimension of AdaHGComputation should be a multiple of 16."
        num_heads = c_ // 16
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.m = AdaHGComputation(embed_dim=c_, num_hyperedges=num_hyperedges, num_heads=num_heads, dropout=0.1, context=context)
        self.cv3 = Conv(2 * c_, c2, 1)

    def _run_cv12(self, x):
        """The stacked cv1|cv2 output (it takes cv1's activation)."""
        return ops.conv2d(self, [L.as_nhwc(x)], lambda: _stacked(self.cv1, self.cv2), 1, 1, 0, _stacked_act(self.cv1), tag="cv12")

    def forward(self, x, out=None, cv12=None):
        """cv12 (extension): the stacked cv1|cv2 output when the caller has already computed it (HyperACE stacks both branches)."""
        c_ = self.cv1.conv.out_channels
        if cv12 is None:
            cv12 = self._run_cv12(x)
        h = self.m(cv12[:, :c_])
        return ops.conv2d(self.cv3, [h, cv12[:, c_:]], self.cv3.folded, 1, 1, 0, _act_code(self.cv3.act), out=out)


class FuseModule(nn.Module):
    """reference block.py:1854-1892: conv_out(cat(avgpool2(x0), x1, up2x(x2))).  The pooled x0 and a copy of x1 share one buffer, which
    conv_out reads together with x2 through its nearest x2 upsample (a two-source 1x1 conv): the concat is never written."""

    def __init__(self, c_in, channel_adjust):
        super(FuseModule, self).__init__()
        self.downsample = nn.AvgPool2d(kernel_size=2)
        self.upsample = nn.Upsample(scale_factor=2, mode="nearest")
        if channel_adjust:
            self.conv_out = Conv(4 * c_in, c_in, 1)
        else:
            self.conv_out = Conv(3 * c_in, c_in, 1)

    def forward(self, x, out=None):
        x0, x1, x2 = (L.as_nhwc(t) for t in x)
        B, c1, H, W = x1.shape
        c0 = x0.shape[1]
        if (x0.shape[2] // 2, x0.shape[3] // 2) != (H, W) or (2 * x2.shape[2], 2 * x2.shape[3]) != (H, W):
            raise ValueError(f"FuseModule: inputs {tuple(x0.shape)}, {tuple(x1.shape)}, {tuple(x2.shape)} do not align at {H}x{W}")
        buf = L.empty_nhwc(B, c0 + c1, H, W, x1.dtype, x1.device)
        ops.avgpool2(x0, out=buf[:, :c0])
        ops.copy_slice(x1, buf[:, c0:])
        c = self.conv_out
        return ops.conv2d(c, [buf, x2], c.folded, 1, 1, 0, _act_code(c.act), out=out, up=[0, 1])


class HyperACE(_Packed):
    """reference block.py:1895-1949: fuse -> cv1 -> [y0, C3AH_1(y1), y2, m chained from y2, C3AH_2(y1)] -> cv2.  Every part is written
    into its slot of one buffer; the four 1x1 convs of the two C3AH branches (all reading y1) run as one stacked launch."""

    def __init__(self, c1, c2, n=1, num_hyperedges=8, dsc3k=True, shortcut=False, e1=0.5, e2=1, context="both", channel_adjust=True):
        super().__init__()
        self.c = int(c2 * e1)
        self.cv1 = Conv(c1, 3 * self.c, 1, 1)
        self.cv2 = Conv((4 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(
            DSC3k(self.c, self.c, 2, shortcut, k1=3, k2=7) if dsc3k else DSBottleneck(self.c, self.c, shortcut=shortcut) for _ in range(n))
        self.fuse = FuseModule(c1, channel_adjust)
        self.branch1 = C3AH(self.c, self.c, e2, num_hyperedges, context)
        self.branch2 = C3AH(self.c, self.c, e2, num_hyperedges, context)

    def forward(self, X, out=None):
        x = self.fuse(X)
        B, _, H, W = x.shape
        c, n = self.c, len(self.m)
        buf = L.empty_nhwc(B, (4 + n) * c, H, W, x.dtype, x.device)  # [y0 | out1 | y2 | m_1 .. m_n | out2]
        self.cv1(x, out=buf[:, :3 * c])
        b1, b2 = self.branch1, self.branch2
        convs = (b1.cv1, b1.cv2, b2.cv1, b2.cv2)
        y1, act = _slot(buf, 1, c), _stacked_act(*convs)
        if act is not None:
            t = ops.conv2d(self, [y1], lambda: _stacked(*convs), 1, 1, 0, act, tag="cv1234")  # [b1.cv1 | b1.cv2 | b2.cv1 | b2.cv2]
            h = b1.cv1.conv.out_channels
            t1, t2 = t[:, :2 * h], t[:, 2 * h:]
        else:
            t1, t2 = b1._run_cv12(y1), b2._run_cv12(y1)
        b1(y1, out=_slot(buf, 1, c), cv12=t1)  # y1 is dead once both branches' 1x1 convs have read it
        b2(y1, out=_slot(buf, 3 + n, c), cv12=t2)
        for i, m in enumerate(self.m):
            m(_slot(buf, 2 + i, c), out=_slot(buf, 3 + i, c))
        return self.cv2(buf, out=out)


class DownsampleConv(nn.Module):
    """reference block.py:1952-1985: channel_adjust(AvgPool2d(2)(x)), a 1x1 Conv c -> 2c or Identity."""

    def __init__(self, in_channels, channel_adjust=True):
        super().__init__()
        self.downsample = nn.AvgPool2d(kernel_size=2)
        if channel_adjust:
            self.channel_adjust = Conv(in_channels, in_channels * 2, 1)
        else:
            self.channel_adjust = nn.Identity()

    def forward(self, x, out=None):
        if isinstance(self.channel_adjust, Conv):
            return self.channel_adjust(ops.avgpool2(x), out=out)
        return ops.avgpool2(x, out=out)


class FullPAD_Tunnel(_Packed):
    """reference block.py:1988-2008: x[0] + gate * x[1] (ey_scale_add_channels with the 0-d gate broadcast, rounded to the activation
    dtype as the reference's product is)."""

    def __init__(self):
        super().__init__()
        self.gate = nn.Parameter(torch.tensor(0.0))

    def forward(self, x, out=None):
        a, t = (L.as_nhwc(v) for v in x)
        return ops.scale_add_channels(a, _scale_vec(self, "gate", self.gate, t), t, out=out)


# ----------------------------------------------------------------------------------------------- YOLOv9 (GELAN)
def _ceil8(c):
    return (c + 7) // 8 * 8


def _pad_folded(fn, out_segs, in_segs):
    """The (BN-folded) weights of `fn()` re-laid on padded channel segments: out_segs / in_segs = [(true width, padded width), ...] in channel
    order; the pad rows, pad columns and pad biases are zero.  yolov9m's hidden widths (60, 90, 180) are no multiples of 8, which the MFMA conv
    and 16-byte channel slots need: its maps carry zero channels at the end of every slot instead (SiLU(0) = 0, so they stay exactly zero and
    add exactly nothing downstream)."""
    def build():
        w, b = fn()
        wp = w.new_zeros((sum(p for _, p in out_segs), sum(p for _, p in in_segs)) + tuple(w.shape[2:]))
        bp = b.new_zeros(wp.shape[0])
        ro = so = 0
        for to, po in out_segs:
            ci = si = 0
            for ti, pi in in_segs:
                wp[ro:ro + to, ci:ci + ti] = w[so:so + to, si:si + ti]
                ci, si = ci + pi, si + ti
            bp[ro:ro + to] = b[so:so + to]
            ro, so = ro + po, so + to
        return wp, bp
    return build


def _conv_padded(conv, x, out, res=None):
    """A Conv / RepConv whose input and output channels are zero-padded at the end to the widths of `x` and `out`."""
    c = conv.conv if hasattr(conv, "conv") else conv.conv1.conv
    k = c.kernel_size[0]
    return ops.conv2d(conv, [x], _pad_folded(conv.folded, [(c.out_channels, out.shape[1])], [(c.in_channels, x.shape[1])]), k, 1, k // 2, _act_code(conv.act),
                      out=out, res=res, tag=f"pad{x.shape[1]}_{out.shape[1]}")


class RepBottleneck(Bottleneck):
    """reference block.py:695-702: a Bottleneck whose first conv is a RepConv."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__(c1, c2, shortcut, g, k, e)
        c_ = int(c2 * e)
        self.cv1 = RepConv(c1, c_, k[0], 1)


class RepCSP(C3):
    """reference block.py:705-712: C3 over RepBottlenecks (same slot scheme as C3: the chain rewrites slot 0 in place)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(RepBottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))

    def forward(self, x, out=None, cv12=None):
        c1, c_, c2 = self.cv1.conv.in_channels, self.cv1.conv.out_channels, self.cv3.conv.out_channels
        if c_ % 8 == 0 and x.shape[1] == c1 and (out is None or out.shape[1] == c2):
            return super().forward(x, out=out, cv12=cv12)
        # zero-padded widths (see _pad_folded): x and out may carry pad channels at the end, the hidden width is padded to a multiple of 8
        if out is None:
            raise NotImplementedError(f"RepCSP: hidden width {c_} is no multiple of 8; built inside RepNCSPELAN4, which supplies the padded output")
        x = L.as_nhwc(x)
        B, xin, H, W = x.shape
        cp = _ceil8(c_)
        buf = ops.conv2d(self, [x], _pad_folded(self._cv12, [(c_, cp), (c_, cp)], [(c1, xin)]), 1, 1, 0, self._cv12_act(), tag=f"cv12pad{xin}")
        slot = buf[:, :cp]
        for b in self.m:
            h = _conv_padded(b.cv1, slot, L.empty_nhwc(B, cp, H, W, x.dtype, x.device))
            _conv_padded(b.cv2, h, slot, res=slot if b.add else None)
        return ops.conv2d(self.cv3, [buf], _pad_folded(self.cv3.folded, [(c2, out.shape[1])], [(c_, cp), (c_, cp)]), 1, 1, 0, _act_code(self.cv3.act), out=out,
                          tag=f"pad{out.shape[1]}")


class RepNCSPELAN4(nn.Module):
    """CSP-ELAN (reference block.py:715-737).  One concat buffer of c3 + 2 c4 channels: cv1 writes the first two slots (c3), cv2 reads the
    second of them and writes the next c4 channels, cv3 reads those and writes the last c4, cv4 reads the buffer in place."""

    def __init__(self, c1, c2, c3, c4, n=1):
        super().__init__()
        self.c = c3 // 2
        self.cv1 = Conv(c1, c3, 1, 1)
        self.cv2 = nn.Sequential(RepCSP(c3 // 2, c4, n), Conv(c4, c4, 3, 1))
        self.cv3 = nn.Sequential(RepCSP(c4, c4, n), Conv(c4, c4, 3, 1))
        self.cv4 = Conv(c3 + (2 * c4), c2, 1, 1)

    @staticmethod
    def _branch(m, x, out):
        if not isinstance(m, nn.Sequential):
            return m(x, out=out)
        B, _, H, W = x.shape  # (RepCSP gets its output buffer: a hidden width that is no multiple of 8 pads inside it, see _pad_folded)
        return m[1](m[0](x, out=L.empty_nhwc(B, m[0].cv3.conv.out_channels, H, W, x.dtype, x.device)), out=out)

    def forward(self, x, out=None):
        B, _, H, W = x.shape  # x may be a VirtualCat (upsample+concat folded into cv1)
        c3 = self.cv1.conv.out_channels
        c, c4 = self.c, (self.cv4.conv.in_channels - c3) // 2
        if c % 8 or c4 % 8:
            return self._forward_padded(x, out, c, c4)
        buf = L.empty_nhwc(B, c3 + 2 * c4, H, W, x.dtype, x.device)
        self.cv1(x, out=buf[:, :c3])
        self._branch(self.cv2, buf[:, c3 - self.c:c3], buf[:, c3:c3 + c4])
        self._branch(self.cv3, buf[:, c3:c3 + c4], buf[:, c3 + c4:])
        return self.cv4(buf, out=out)

    def _forward_padded(self, x, out, c, c4):
        """Widths that are no multiples of 8 (yolov9m: 180 | 180 | 180 | 180): every slot of the buffer is padded with zero channels to the next
        multiple of 8 (see _pad_folded); cv4's weights skip them."""
        B, _, H, W = x.shape
        hp, qp = _ceil8(c), _ceil8(c4)
        buf = L.empty_nhwc(B, 2 * hp + 2 * qp, H, W, x.dtype, x.device)
        c1 = self.cv1.conv.in_channels
        ops.conv2d(self.cv1, [x], _pad_folded(self.cv1.folded, [(c, hp), (c, hp)], [(c1, c1)]), 1, 1, 0, _act_code(self.cv1.act), out=buf[:, :2 * hp], tag="pad")
        src = buf[:, hp:2 * hp]
        for i, m in enumerate((self.cv2, self.cv3)):
            dst = buf[:, 2 * hp + i * qp:2 * hp + (i + 1) * qp]
            if isinstance(m, nn.Sequential):
                _conv_padded(m[1], m[0](src, out=L.empty_nhwc(B, qp, H, W, x.dtype, x.device)), dst)
            else:
                _conv_padded(m, src, dst)
            src = dst
        c2 = self.cv4.conv.out_channels
        return ops.conv2d(self.cv4, [buf], _pad_folded(self.cv4.folded, [(c2, c2)], [(c, hp), (c, hp), (c4, qp), (c4, qp)]), 1, 1, 0, _act_code(self.cv4.act),
                          out=out, tag="pad")

    forward_split = forward


class ELAN1(RepNCSPELAN4):
    """reference block.py:740-750: RepNCSPELAN4 whose two branches are plain 3x3 convs."""

    def __init__(self, c1, c2, c3, c4):
        super().__init__(c1, c2, c3, c4)
        self.c = c3 // 2
        self.cv1 = Conv(c1, c3, 1, 1)
        self.cv2 = Conv(c3 // 2, c4, 3, 1)
        self.cv3 = Conv(c4, c4, 3, 1)
        self.cv4 = Conv(c3 + (2 * c4), c2, 1, 1)


class AConv(nn.Module):
    """reference block.py:753-764: avg_pool2d(x, 2, 1, 0) (ey_adown_pool, AConv mode) -> 3x3 stride-2 conv."""

    def __init__(self, c1, c2):
        super().__init__()
        self.cv1 = Conv(c1, c2, 3, 2, 1)

    def forward(self, x, out=None):
        a, _ = ops.adown_pool(x)
        return self.cv1(a, out=out)


class ADown(nn.Module):
    """reference block.py:767-784.  ONE ey_adown_pool launch gives the averaged first half and the averaged-then-max-pooled second half (the
    averaged second half is never written); cv1 (3x3 stride 2) and cv2 (1x1) write the two halves of the output buffer."""

    def __init__(self, c1, c2):
        super().__init__()
        self.c = c2 // 2
        self.cv1 = Conv(c1 // 2, self.c, 3, 2, 1)
        self.cv2 = Conv(c1 // 2, self.c, 1, 1, 0)

    def forward(self, x, out=None):
        B, c1, H, W = x.shape
        a, m = ops.adown_pool(x, c1 // 2)
        if out is None:
            out = L.empty_nhwc(B, 2 * self.c, H // 2, W // 2, x.dtype, x.device)
        self.cv1(a, out=out[:, :self.c])
        self.cv2(m, out=out[:, self.c:])
        return out


class SPPELAN(nn.Module):
    """reference block.py:787-804: cv1 -> three chained 5x5 max-pools (ONE ey_sppf_pool launch into slots 1-3 of a 4 c3 buffer) -> cv5.
    cv2-cv4 are the reference's nn.MaxPool2d children (no parameters; never called)."""

    def __init__(self, c1, c2, c3, k=5):
        super().__init__()
        if k != 5:
            raise NotImplementedError("SPPELAN pooling kernel is built for k=5 (the only value the YAMLs use)")
        self.c = c3
        self.cv1 = Conv(c1, c3, 1, 1)
        self.cv2 = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)
        self.cv3 = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)
        self.cv4 = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)
        self.cv5 = Conv(4 * c3, c2, 1, 1)

    def forward(self, x, out=None):
        return _pool_pyramid(self.cv1, self.cv5, x, out)


class CBLinear(_Packed):
    """reference block.py:807-818: ONE 1x1 conv with bias (no BatchNorm, no activation); the outputs are channel-slice views of it."""

    def __init__(self, c1, c2s, k=1, s=1, p=None, g=1):
        super().__init__()
        if k != 1 or s != 1 or g != 1:
            raise NotImplementedError(f"CBLinear(k={k}, s={s}, g={g}): only the pointwise form (k=1, s=1, g=1) of the YOLOv9 YAMLs is built")
        self.c2s = list(c2s)
        self.conv = nn.Conv2d(c1, sum(c2s), k, s, k // 2 if p is None else p, groups=g, bias=True)

    def _folded(self):
        return fold_bn(self.conv.weight, self.conv.bias, None)

    def forward(self, x):
        y = ops.conv2d(self, [x], self._folded, 1, 1, 0, L.ACT_NONE)
        outs, o = [], 0
        for c in self.c2s:
            outs.append(y[:, o:o + c])
            o += c
        return tuple(outs)


class CBFuse(nn.Module):
    """reference block.py:821-833: sum of xs[i][idx[i]] nearest-resized to the last input's size, plus that input -- ONE ey_cbfuse launch
    (fp32 sum in list order, one rounding)."""

    def __init__(self, idx):
        super().__init__()
        self.idx = idx

    def forward(self, xs):
        if len(xs) > L.CBFUSE_MAX:
            raise NotImplementedError(f"CBFuse: {len(xs)} inputs; ey_cbfuse takes at most {L.CBFUSE_MAX}")
        return ops.cbfuse([x[self.idx[i]] for i, x in enumerate(xs[:-1])] + [xs[-1]])


# ----------------------------------------------------------------------------------------------- YOLOv10
class SCDown(nn.Module):
    """Spatial-channel decoupled downsampling of YOLOv10 (reference block.py:1174-1206): cv2(cv1(x)), cv1 a pointwise Conv + SiLU, cv2 a
    depthwise k x k stride-s Conv without activation.  Stride 2 runs as ONE kernel where the shape allows (ops.scdown: the full-resolution
    c2-channel map stays in LDS), else as ey_conv2d + ey_dwconv_s2 -- the same bits either way.  `out=` may be a slot of a concat buffer."""

    def __init__(self, c1, c2, k, s):
        super().__init__()
        self.cv1 = Conv(c1, c2, 1, 1)
        self.cv2 = Conv(c2, c2, k=k, s=s, g=c2, act=False)

    def forward(self, x, out=None):
        c = self.cv2.conv
        k = c.kernel_size[0]
        if c.stride == (2, 2) and k in (3, 5, 7) and c.kernel_size == (k, k) and c.padding == (k // 2, k // 2) and c.dilation == (1, 1):
            y = ops.scdown(self.cv1, self.cv2, x, out=out)
            if y is not None:
                return y
            return ops.dwconv_s2(self.cv2, self.cv1(x), self.cv2.folded, k, _act_code(self.cv2.act), out=out)
        return self.cv2(self.cv1(x), out=out)


class RepVGGDW(_Packed):
    """Re-parameterised depthwise block of the YOLOv10 CIB (reference block.py:879-938): SiLU(conv 7x7 dw (x) + conv1 3x3 dw (x)), both
    Conv(act=False).  The two branches are linear in x, so the HIP path always runs ONE depthwise 7x7 on the sum of the 7x7 kernel and the
    3x3 kernel padded to 7x7 (biases added), BatchNorms folded in fp32 when the weights are packed -- before `fuse()` (from conv / conv1) and
    after it (from the single `conv` with bias it leaves)."""

    def __init__(self, ed):
        super().__init__()
        self.conv = Conv(ed, ed, 7, 1, 3, g=ed, act=False)
        self.conv1 = Conv(ed, ed, 3, 1, 1, g=ed, act=False)
        self.dim = ed
        self.act = nn.SiLU()

    def folded(self):
        """(7x7 depthwise kernel (ed,1,7,7), bias) equal to both branches, in fp32 (reference :921-932)."""
        if not hasattr(self, "conv1"):
            return self.conv.weight.detach().float(), self.conv.bias.detach().float()
        k7, b7 = self.conv.folded()
        k3, b3 = self.conv1.folded()
        return k7 + F.pad(k3, [2, 2, 2, 2]), b7 + b3

    @torch.no_grad()
    def fuse(self):
        """Leave a single `conv` (nn.Conv2d with bias) and drop conv1 (reference :914-938)."""
        if not hasattr(self, "conv1"):
            return
        w, b = self.folded()
        c, dt = self.conv.conv, self.conv.conv.weight.dtype
        conv = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.dilation, c.groups, bias=True).requires_grad_(False)
        conv = conv.to(w.device)
        conv.weight.data = w.to(dt)
        conv.bias.data = b.to(dt)
        self.conv = conv
        del self.conv1
        self._cache = {}

    def forward(self, x, out=None):
        return ops.dwconv(self, x, self.folded, 7, _act_code(self.act), out=out)

    forward_fuse = forward


class CIB(nn.Module):
    """Compact inverted block of YOLOv10 (reference block.py:941-977): dw 3x3 -> pw (c1 -> 2c_) -> dw 3x3 (RepVGGDW 7x7 with lk) -> pw
    (2c_ -> c2) -> dw 3x3, every stage + SiLU, plus x when shortcut and c1 == c2.  Five launches on the depthwise and MFMA pointwise
    kernels; the last stage is a depthwise kernel, which has no residual input, so the add is ey_cbfuse on two maps (x + y in fp32, one
    rounding)."""

    def __init__(self, c1, c2, shortcut=True, e=0.5, lk=False):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = nn.Sequential(
            Conv(c1, c1, 3, g=c1),
            Conv(c1, 2 * c_, 1),
            RepVGGDW(2 * c_) if lk else Conv(2 * c_, 2 * c_, 3, g=2 * c_),
            Conv(2 * c_, c2, 1),
            Conv(c2, c2, 3, g=c2),
        )
        self.add = shortcut and c1 == c2

    def forward(self, x, out=None):
        m = self.cv1
        t = m[3](m[2](m[1](m[0](x))))
        if not self.add:
            return m[4](t, out=out)
        return ops.cbfuse([x, m[4](t)], out=out)


class C2fCIB(C2f):
    """C2f with CIB blocks in place of the bottlenecks (reference block.py:980-997)."""

    def __init__(self, c1, c2, n=1, shortcut=False, lk=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(CIB(self.c, self.c, shortcut, e=1.0, lk=lk) for _ in range(n))


class PSA(nn.Module):
    """Partial self-attention of YOLOv10 (reference block.py:1057-1097): cv1 splits into (a, b); b = b + attn(b); b = b + ffn(b);
    cv2(cat(a, b)).  Both residual adds ride in conv epilogues and b is updated in its half of cv1's buffer: no split, add or cat kernel.
    c // 64 heads of head_dim 64 / key_dim 32 where c is a multiple of 64 (2 at n, 5 at x); 4 heads of 72 / 36 at the m scale (c = 288)."""

    def __init__(self, c1, c2, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.attn = Attention(self.c, attn_ratio=0.5, num_heads=self.c // 64)
        self.ffn = nn.Sequential(Conv(self.c, self.c * 2, 1), Conv(self.c * 2, self.c, 1, act=False))

    def forward(self, x, out=None):
        t = self.cv1(x)
        _attn_ffn(self.attn, self.ffn, t[:, self.c:], out=t[:, self.c:])
        return self.cv2(t, out=out)


# ----------------------------------------------------------------------------------------------- YOLOv8 (P6 heads) and YOLOv8-ghost
class C2(nn.Module):
    """CSP bottleneck with two convolutions (reference block.py:339-354): cv2(cat(m(a), b)) with (a, b) = cv1(x).chunk(2), m a chain of
    3x3 + 3x3 Bottlenecks -- the head blocks of yolov8-p6.yaml.  The chain rewrites a's half of cv1's buffer in place (a Bottleneck's
    closing conv reads a temporary and adds its input pixel by pixel as the residual), so there is no chunk and no cat."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n)))

    def forward(self, x, out=None):
        buf = self.cv1(x)  # x may be a VirtualCat (upsample + concat folded into cv1)
        a = buf[:, :self.c]
        for m in self.m:
            m(a, out=a)
        return self.cv2(buf, out=out)


class GhostBottleneck(nn.Module):
    """Ghost bottleneck (reference block.py:446-464): conv(x) + shortcut(x), conv = GhostConv(c1, c2 / 2) -> [DWConv k x k stride 2] ->
    GhostConv(c2 / 2, c2, act=False).  Stride 1 (every shipped YAML): the shortcut is x itself and rides in the closing GhostConv's kernel
    (`res=`), so the block is two launches, and `out=` may be x (C3Ghost's in-place chain).  Stride 2: the shortcut is DWConv stride 2 ->
    Conv 1x1, composed from the existing kernels."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(
            GhostConv(c1, c_, 1, 1),
            DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
            GhostConv(c_, c2, 1, 1, act=False),
        )
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False), Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()

    def forward(self, x, out=None):
        t = self.conv[0](x)
        if isinstance(self.shortcut, nn.Identity):
            if t.shape[1] * 2 != x.shape[1]:
                raise ValueError(f"GhostBottleneck: the stride-1 block adds its input, which needs c1 == c2 (got {x.shape[1]} and {t.shape[1] * 2})")
            return self.conv[2](t, out=out, res=x)
        return self.conv[2](self.conv[1](t), out=out, res=self.shortcut[1](self.shortcut[0](x)))


class C3Ghost(C3):
    """C3 with GhostBottlenecks (reference block.py:436-443), on C3's concat buffer: the chain rewrites slot 0 in place."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(GhostBottleneck(c_, c_) for _ in range(n)))


class ResNetBlock(_Packed):
    """Bottleneck block of the ResNets (reference block.py:505-519): relu(cv3(cv2(cv1(x))) + shortcut(x)), cv1 1x1 and cv2 3x3 (stride s) with the
    default activation, cv3 1x1 to e c2 channels and the shortcut -- a 1x1 stride-s Conv where the shape changes, else the identity -- without
    one.  The sum comes BEFORE the ReLU, so it is not the `res=` of ey_conv2d (added behind the activation).  The closing launch is
      * fused (f16): ONE ey_resnet_tail launch.  A projection block reads t = cv2(cv1(x)) and x at pixel stride s against [W3 | Ws]
        concatenated along K with the bias b3 + bs -- the shortcut conv's output never exists --, an identity block adds the block input in
        fp32 before the ReLU; one rounding either way;
      * composed (fp32 always, and every shape the kernel refuses): the shortcut conv where the block has one, then cv3 on ey_conv2d with
        ReLU and the shortcut (or the block input) as its pre-activation term `addz` at the output's own size, where the bilinear index
        arithmetic of that term gives the weights exactly 1 and 0.
    `tail_fused` = True / False forces a form where the kernel takes the shape; "auto" (the default) follows the measurement on MI355X at
    batch 32, f16, 224 x 224 (profiles/resnet_bench.txt): `fused_shapes` lists the (c1 or 0, c2) pairs at which the fused
    kernel was faster than the composed form by more than the spread; every other shape takes the composed form.  The list is keyed on the
    channel widths alone and comes from that one operating point: it is not re-derived for other batch or map sizes."""

    tail_fused = "auto"
    # (c1, c2) of projection blocks / (0, c2) of identity blocks.  Fused against composed, us: (64, 64) at 56 x 56 53.7 / 89.5 -- taken; (256, 128)
    # stride 2 64.4 / 64.4, (512, 256) 69.4 / 47.5, (1024, 512) 68.1 / 52.2, identity 64: 58.1 / 54.3, 128: 40.2 / 34.2, 256: 33.8 / 23.9, 512: 29.6 / 18.0
    fused_shapes = frozenset({(64, 64)})

    def __init__(self, c1, c2, s=1, e=4):
        super().__init__()
        c3 = e * c2
        self.cv1 = Conv(c1, c2, k=1, s=1, act=True)
        self.cv2 = Conv(c2, c2, k=3, s=s, p=1, act=True)
        self.cv3 = Conv(c2, c3, k=1, act=False)
        self.shortcut = nn.Sequential(Conv(c1, c3, k=1, s=s, act=False)) if s != 1 or c1 != c3 else nn.Identity()

    def _tail_folded(self):
        w3, b3 = self.cv3.folded()
        if not isinstance(self.shortcut, nn.Sequential):
            return w3, b3
        ws, bs = self.shortcut[0].folded()
        return torch.cat([w3, ws], 1), b3 + bs

    def tail(self, t, x, out=None):
        """relu(cv3(t) + shortcut(x)) for t = cv2(cv1(x))."""
        proj = isinstance(self.shortcut, nn.Sequential)
        fused = self.tail_fused
        if fused == "auto":
            fused = ((self.shortcut[0].conv.in_channels if proj else 0), t.shape[1]) in self.fused_shapes
        if fused and torch.is_tensor(x) and x.dtype == torch.float16 and self.cv3.conv.out_channels == 4 * t.shape[1]:
            # (the cache slot names the fused state: fuse() rewrites the parameters of cv3 and the shortcut, whose own caches it drops)
            y = ops.resnet_tail(self, t, x, self._tail_folded, self.shortcut[0].conv.stride[0] if proj else 1, not proj, out=out, tag=str(int(hasattr(self.cv3, "bn"))))
            if y is not None:
                return y
        z = self.shortcut[0](x) if proj else ops.as_tensor(x)
        return ops.conv2d(self.cv3, [t], self.cv3.folded, 1, 1, 0, L.ACT_RELU, out=out, addz=z)

    def forward(self, x, out=None):
        return self.tail(self.cv2(self.cv1(x)), x, out=out)


class ResNetLayer(nn.Module):
    """One stage of a ResNet (reference block.py:522-541), args (c1, c2, s, is_first, n, e).  `is_first`: the stem, Conv(c1, c2, 7, 2, 3) from the
    planar image and nn.MaxPool2d(3, 2, 1) (the torch module is a parameter-free place holder that keeps the reference's `layer.0` /
    `layer.1` numbering and is never called).  Two forms with the same bits: ONE ey_resnet_stem launch (the half-resolution map stays in LDS),
    or ey_stem_conv_ks + ey_maxpool3x3s2.  `stem_fused` = True / False forces a form where the kernel takes the shape; "auto" (the default)
    follows the measurement on MI355X at batch 32, f16 (profiles/resnet_bench.txt).  Otherwise n ResNetBlocks, the
    first with stride s."""

    stem_fused = "auto"
    # what "auto" takes.  Batch 32, f16: one ey_resnet_stem launch 101.4 us at 224 x 224 and 815.2 us at 640 x 640 against 60.1 and 428.5 us for the two
    # launches (one workgroup per CU beside its 83 KiB LDS tile, a quarter of the conv tile recomputed or unused): not faster, so the pair is taken
    stem_fused_auto = False

    def __init__(self, c1, c2, s=1, is_first=False, n=1, e=4):
        super().__init__()
        self.is_first = is_first
        if self.is_first:
            self.layer = nn.Sequential(Conv(c1, c2, k=7, s=2, p=3, act=True), nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
        else:
            blocks = [ResNetBlock(c1, c2, s, e=e)]
            blocks.extend([ResNetBlock(e * c2, c2, 1, e=e) for _ in range(n - 1)])
            self.layer = nn.Sequential(*blocks)

    def forward(self, x, out=None):
        ops._no_block("ResNetLayer")
        if self.is_first:
            conv = self.layer[0]
            fused = self.stem_fused_auto if self.stem_fused == "auto" else self.stem_fused
            if fused and torch.is_tensor(x) and x.dim() == 4 and x.is_contiguous() and not L.is_nhwc_view(x) and conv.conv.groups == 1:
                y = ops.resnet_stem(conv, x, conv.folded, _act_code(conv.act), out=out)
                if y is not None:
                    return y
            return ops.maxpool3x3s2(conv(x), out=out)
        for i, b in enumerate(self.layer):
            x = b(x, out=out if i == len(self.layer) - 1 else None)
        return x
