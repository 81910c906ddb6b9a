"""Detection heads, HIP-backed: `Detect` (reference head.py:38-189), `Segment` (:347-369), `OBB` (:372-399), `Pose` (:402-451), `Classify` (:454-476), `WorldDetect` (:479-521), `GF2Detect` (:194-345), `E2EDetect` (:799-824),
`GFLHeadv2_uniH` (:827-908).  Same constructor signatures / attribute names / state_dict keys.  The towers are MFMA convs and
depthwise kernels; everything after them (DGQP statistics + quality FCs, DFL softmax-expectation, anchor decode,
score modulation) is ONE fused kernel per pyramid level writing the (B, 4+nc, A) fp32 prediction tensor.

Host structure: module-level builders make the towers the heads share; `Detect._run_towers` is the one fork / join over HIP streams
(`_stream_map` places the towers); `_padded` allocates a level's map, `Detect._levels` makes the `_ops.Level` list the decode kernels
take; the towers' branch ("" or "one2one_") is an argument of whatever reads weights, and caches are keyed by what an entry is.
"""
import copy
import math
from functools import partial

import torch
import torch.nn as nn

from .block import DFL, Proto
from .conv import Conv, DWConv, _Packed, _act_code, fold_bn
from .. import _ops as ops
from ... import _lib as L
from ...utils.ops import _class_mask

__all__ = ("Detect", "Segment", "OBB", "Pose", "Classify", "GF2Detect", "E2EDetect", "GFLHeadv2_uniH", "WorldDetect", "v10Detect")


class _Plain(_Packed):
    """Weights of a bare nn.Conv2d(+bias) 1x1 tower tail, packed for the MFMA conv."""

    def __init__(self, conv):
        super().__init__()
        self.__dict__["_ref"] = conv  # not registered: the nn.Conv2d stays where the reference keeps it

    def folded(self):
        c = self._ref
        return fold_bn(c.weight, c.bias, None)

    def run(self, x, out):
        return ops.conv2d(self, [x], self.folded, 1, 1, 0, L.ACT_NONE, out=out)


def _plain_towers(ch, c, cout):
    """One Conv 3x3 -> Conv 3x3 -> nn.Conv2d 1x1 tower per level: the box tower (head.py:60-62), the legacy class tower (:64) and every cv4."""
    return nn.ModuleList(nn.Sequential(Conv(x, c, 3), Conv(c, c, 3), nn.Conv2d(c, cout, 1)) for x in ch)


def _light_towers(ch, c3, nc):
    """The light class tower per level (head.py:66-74): DWConv -> Conv 1x1 -> DWConv -> Conv 1x1 -> nn.Conv2d 1x1."""
    return nn.ModuleList(
        nn.Sequential(nn.Sequential(DWConv(x, x, 3), Conv(x, c3, 1)), nn.Sequential(DWConv(c3, c3, 3), Conv(c3, c3, 1)), nn.Conv2d(c3, nc, 1))
        for x in ch)


def _reg_conf(ch, reg_topk, add_mean, reg_channels):
    """The DGQP quality head per level (head.py:211-219)."""
    in_stat = 4 * (reg_topk + (1 if add_mean else 0))
    return nn.ModuleList(
        nn.Sequential(nn.Conv2d(in_stat, reg_channels, 1, bias=True), nn.ReLU(inplace=True), nn.Conv2d(reg_channels, 1, 1, bias=True), nn.Sigmoid())
        for _ in ch)


def _light_closing(c):
    """Does the class tower `c` close as the light tower does: Sequential(DWConv, Conv 1x1 + SiLU), then a dense nn.Conv2d 1x1?"""
    last, ct = c[-2], c[-1]
    return (isinstance(last, nn.Sequential) and len(last) == 2 and isinstance(last[0], DWConv) and isinstance(last[1], Conv)
            and last[1].conv.kernel_size == (1, 1) and last[1].conv.groups == 1 and isinstance(last[1].act, nn.SiLU)
            and isinstance(ct, nn.Conv2d) and ct.kernel_size == (1, 1) and ct.groups == 1)


def _padded(t, c):
    """An NHWC map of `c` channels over the pixels of `t` whose pixel stride is rounded up to 8 channels (kept 16-byte aligned for any c)."""
    return L.empty_nhwc(t.shape[0], (c + 7) // 8 * 8, t.shape[2], t.shape[3], t.dtype, t.device)[:, :c]


class Detect(nn.Module):
    """YOLO Detect head (reference head.py:38-189)."""

    dynamic = False
    export = False
    format = None
    end2end = False
    max_det = 300
    shape = None
    anchors = torch.empty(0)
    strides = torch.empty(0)
    legacy = False
    # Execution options (instance attributes; they never change results):
    #  head_streams: run the towers of the smaller pyramid levels on a second HIP stream (a parallel hipGraph branch).  A caller
    #                that already runs the head as a pipeline stage of its own (YOLO.predict_batches, bench.py) sets it False.
    #  tower_streams: optional stream index (0 = the caller's stream) per tower in order (level0 box, level0 cls, level1 box, ...)
    #  chain: fuse the last two 1x1 convs of the class tower into one register-only kernel (ey_conv_pw_chain)
    head_streams = True
    tower_streams = None
    chain = True
    #  block_fusion: both towers of a pyramid level whose map has at most block_max_pixels pixels (20x20 at 640x640) run as ONE block
    #                program (nn/_block.py: one persistent workgroup per image) instead of 7 launches; f16 mode only.  Opt-in: measured
    #                slower than the per-layer kernels at batch 32 (see DetectionModel.block_fusion)
    block_fusion = False
    block_max_pixels = 1024

    def __init__(self, nc=80, ch=()):
        super().__init__()
        self.nc = nc
        self.nl = len(ch)
        self.reg_max = 16
        self.no = nc + self.reg_max * 4
        self.stride = torch.zeros(self.nl)
        c2, c3 = max((16, ch[0] // 4, self.reg_max * 4)), max(ch[0], min(self.nc, 100))
        self.cv2 = _plain_towers(ch, c2, 4 * self.reg_max)
        self.cv3 = _plain_towers(ch, c3, self.nc) if self.legacy else _light_towers(ch, c3, self.nc)
        self.dfl = DFL(self.reg_max) if self.reg_max > 1 else nn.Identity()
        if self.end2end:  # head.py:76-78
            self.one2one_cv2 = copy.deepcopy(self.cv2)
            self.one2one_cv3 = copy.deepcopy(self.cv3)
        self._tails = {}
        # packed tails / quality-head weights are caches of parameters: drop them whenever parameters are (re)loaded
        self.register_load_state_dict_post_hook(lambda m, _keys: m._reset_caches())

    def _reset_caches(self):
        self.__dict__["_blk"] = {}
        self._tails = {}
        self._stride_f = None
        if hasattr(self, "_qcache"):
            self._qcache = {}

    def _apply(self, fn, *a, **k):
        self._reset_caches()
        return super()._apply(fn, *a, **k)

    def _refuse(self, head=None):
        """The refusals that open a forward: training mode, and (`head` = the class's name) end2end where that head has no such path."""
        if self.training:
            raise RuntimeError("edge-yolo_amd implements the inference forward only: call model.eval()")
        if head and self.end2end:
            raise NotImplementedError(f"{head}: end2end heads are not built")

    # ---- towers.  `branch` = which towers' weights run: "" (cv2 / cv3 / reg_conf) or "one2one_" (their end2end copies, head.py:76-78,220-221)
    def _tail(self, tower, i, branch=""):
        """The packed closing nn.Conv2d of level i's `tower` ("cv2" / "cv3" / "cv4")."""
        key = (branch, tower, i)
        t = self._tails.get(key)
        if t is None:
            t = self._tails[key] = _Plain(getattr(self, branch + tower)[i][-1])
        return t

    def _box_tower(self, i, x, raw, branch=""):
        """box logits -> raw[:, :64]."""
        b = getattr(self, branch + "cv2")[i]
        self._tail("cv2", i, branch).run(b[1](b[0](x)), raw[:, :4 * self.reg_max])

    def _chained(self, i, x, branch=""):
        """non-legacy tower (head.py:68-70): ... -> DWConv -> Conv(c3,c3,1)+SiLU -> nn.Conv2d(c3,nc,1): the last two 1x1 convs run as ONE
        register-only kernel when the shape fits (ey_conv_pw_chain), the intermediate (B,c3,H,W) tensor never exists."""
        return self.chain and x.dtype == torch.float16 and _light_closing(getattr(self, branch + "cv3")[i])

    def _cls_stem(self, i, x, chained, branch="", out=None):
        """The class tower of level i up to its closing (`_cls_close`): chained, up to and including the last DWConv (into `out` when
        given); else everything but the nn.Conv2d."""
        c = getattr(self, branch + "cv3")[i]
        for j in range(len(c) - (2 if chained else 1)):
            x = c[j](x)  # (ops.dsconv fuses DWConv+Conv into one kernel; measured slower than the two kernels at these widths)
        return c[-2][0](x, out=out) if chained else x

    def _cls_close(self, i, t, out, chained, branch=""):
        """The closing of level i's class tower: `_cls_stem`'s feature -> class logits in `out`."""
        tail = self._tail("cv3", i, branch)
        if chained:
            pw = getattr(self, branch + "cv3")[i][-2][1]
            if ops.conv_pw_chain(tail, t, pw.folded, L.ACT_SILU, tail.folded, L.ACT_NONE, out) is not None:
                return
            t = pw(t)
        tail.run(t, out)

    def _cls_tower(self, i, x, raw, out=None, branch=""):
        """class logits -> raw[:, 64:] (or `out`)."""
        chained = self._chained(i, x, branch)
        self._cls_close(i, self._cls_stem(i, x, chained, branch), raw[:, 4 * self.reg_max:] if out is None else out, chained, branch)

    def _towers(self, i, x, raw, branch=""):
        self._box_tower(i, x, raw, branch)
        self._cls_tower(i, x, raw, branch=branch)

    def _towers_block(self, i, x, raw):
        """Both towers of level i as one block program; False when the level is not block-executable (per-layer kernels then)."""
        if not self.block_fusion or x.dtype != torch.float16 or x.shape[2] * x.shape[3] > self.block_max_pixels or x.shape[0] < 2:
            return False
        from .._block import BlockCache
        cache = self.__dict__.setdefault("_blk", {}).get(i)
        if cache is None:
            cache = self._blk[i] = BlockCache(f"head level {i}")

        def chain(t):
            self._towers(i, t, raw)
            return [raw]

        return cache.run(chain, [x], [raw]) is not None

    def _level_towers(self, i, x, raw):
        """Both towers of level i on one stream: small levels go through one block program."""
        if not self._towers_block(i, x, raw):
            self._towers(i, x, raw)

    def _stream_map(self, n):
        """Stream index (0 = the caller's stream) of each of the 2n towers, in the order of `tower_streams`."""
        ts = self.tower_streams
        # default: the first (largest) level on the caller's stream, all smaller levels one after the other on ONE side stream
        return list(ts) if ts and len(ts) == 2 * n else [0, 0] + [1] * (2 * n - 2)

    def _run_towers(self, tasks, smap, dev):
        """tasks: [(tower number = 2 * level + (0 box | 1 class), callable)] in launch order; each runs on the stream `smap` gives its tower.
        The towers of the pyramid levels are independent: the small levels run on a second HIP stream (fork / join around them),
        which a captured hipGraph records as a parallel branch -- the 20x20 and 40x40 towers (a few hundred workgroups per kernel)
        then run beside the 80x80 ones instead of after them (2.18 -> 2.08 ms/step).  More branches are slower (3 level streams
        2.38 ms, 6 tower streams 2.40 ms: the persistent kernels fight for the CUs).  `head_streams = False` keeps one stream.
        The caller allocates every buffer a side stream WRITES before this call, that is before the fork: a block handed out later on
        the caller's stream could be one that kernels still queued there are using (the caching allocator orders reuse per stream only)."""
        if not (self.head_streams and dev.type == "cuda" and len(smap) > 2):
            for _, run in tasks:
                run()
            return
        if getattr(self, "_side", None) is None or self._side_dev != dev or len(self._side) != max(smap):
            self._side, self._side_dev = [torch.cuda.Stream(device=dev) for _ in range(max(smap))], dev
        cur = torch.cuda.current_stream(dev)
        for side in self._side:
            side.wait_stream(cur)
        for k, run in tasks:
            if smap[k] > 0:
                with torch.cuda.stream(self._side[smap[k] - 1]):
                    run()
            else:
                run()
        for side in self._side:
            cur.wait_stream(side)

    # ---- levels
    def _quality_params(self, i, device, branch=""):
        return None

    def _walk(self, maps):
        """[(stride, first anchor)] of the per-level maps, in order."""
        if getattr(self, "_stride_f", None) is None:
            self._stride_f = [float(s) for s in self.stride]  # host copy once (no D2H inside a captured graph)
        walk, a_off = [], 0
        for i, m in enumerate(maps):
            walk.append((self._stride_f[i], a_off))
            a_off += m.shape[2] * m.shape[3]
        return walk

    def _split(self, raw):
        return raw[:, :4 * self.reg_max], raw[:, 4 * self.reg_max:]

    def _levels(self, maps, branch=""):
        """Per-level (box map, class map) pairs -> the decode kernels' level list."""
        walk = self._walk([box for box, _ in maps])
        return [ops.Level(box, cls, st, self._quality_params(i, box.device, branch), off) for i, ((box, cls), (st, off)) in enumerate(zip(maps, walk))]

    def forward(self, x, nms=None, towers_only=False):
        """towers_only (subclasses that decode themselves, OBB): stop behind the towers and return (levels, raw maps) as `defer_decode` does.
        nms=None: returns (pred (B,4+nc,A) fp32, raw per-level maps) like the reference.  nms=dict(conf=, classes=None, keep_pred=False)
        (predict pipelines): the decode also builds the NMS candidates for that confidence threshold / class filter in the same pass
        and returns (_ops.Candidates, raw maps) -- `utils.ops.nms_device` takes it in place of `pred`, which is then neither written nor
        re-read (keep_pred=True still writes it, as Candidates.pred).  Where the head has the standard shape (f16, 64-channel box
        tower, class chain c3 -> 80 -> nc with nc % 8 == 0, 64 < nc <= 80) the closing 1x1 convs of both towers run inside the decode
        kernel (tunable head_fuse): their logits are then never written, and the second return value holds None per level -- pass
        nms["keep_raw"]=True to keep the separate launches and get the raw maps."""
        self._refuse()
        if self.reg_max != 16:
            raise NotImplementedError("the decode kernel is built for reg_max=16")
        xs = [L.as_nhwc(t) for t in x]
        if self.end2end:
            return self._forward_end2end(x, xs)
        B, dev = xs[0].shape[0], xs[0].device
        A = sum(t.shape[2] * t.shape[3] for t in xs)
        want_pred = not towers_only and (nms is None or nms.get("keep_pred") or not (len(xs) <= 4 and self.nc > 1))
        pred = torch.empty((B, 4 + self.nc, A), dtype=torch.float32, device=dev) if want_pred else None
        smap = self._stream_map(len(xs))
        fuse = self._head_fuse(xs, nms)
        if fuse:
            return self._forward_fused(xs, nms, fuse, pred, smap)
        raws = [_padded(t, self.no) for t in xs]
        tasks = []
        for i, (t, raw) in enumerate(zip(xs, raws)):
            if smap[2 * i] == smap[2 * i + 1]:
                tasks.append((2 * i, partial(self._level_towers, i, t, raw)))
            else:
                tasks += [(2 * i, partial(self._box_tower, i, t, raw)), (2 * i + 1, partial(self._cls_tower, i, t, raw))]
            x[i] = raw
        self._run_towers(tasks, smap, dev)
        levels = self._levels([self._split(raw) for raw in raws])
        if towers_only or getattr(self, "defer_decode", False):
            # two-stage pipelines (engine/predictor.py::PipelinedRunner) put the decode into the post-processing stage, next to the
            # NMS: the next batch's backbone then starts as soon as the towers are done instead of behind the decode launch
            return levels, x
        if nms is not None and len(levels) <= 4 and self.nc > 1:
            classes = nms.get("classes")
            cand = ops.head_decode_levels(levels, pred if nms.get("keep_pred") else None, nms=(nms["conf"], self._class_mask(classes, dev), classes))
            return cand, x
        self._decode(levels, pred)
        return pred if self.export else (pred, x)

    def _class_mask(self, classes, dev):
        return _class_mask(classes, self.nc, dev)

    # ---- predict mode: the towers' closing 1x1 convs inside the decode kernel (ey_head_tail_decode_levels_nms)
    def _head_fuse(self, xs, nms, branch=""):
        """0 = the towers write their logits and the decode reads them; 1 = the box tail (nn.Conv2d(64, 64, 1)) runs inside the decode
        kernel; 2 = so does the class chain (Conv(c3, 80, 1) + SiLU -> nn.Conv2d(80, nc, 1)).  The tunable head_fuse (csrc/tune.h) picks the
        level; the structure and shape gate below mirrors the kernel's."""
        if (nms is None or nms.get("keep_raw") or getattr(self, "defer_decode", False) or self.block_fusion or not self.chain or self.legacy
                or len(xs) > 4 or xs[0].dtype != torch.float16 or self.nc % 8 or not 64 < self.nc <= 80 or xs[0].device.type != "cuda"):
            return 0
        fuse = int(L.lib().ey_tune_get(b"head_fuse"))
        if fuse not in (1, 2):
            return 0
        for i in range(len(xs)):
            b, c = getattr(self, branch + "cv2")[i], getattr(self, branch + "cv3")[i]
            if not (len(b) == 3 and isinstance(b[1], Conv) and isinstance(b[2], nn.Conv2d) and b[2].kernel_size == (1, 1) and b[2].groups == 1
                    and b[2].in_channels == 64 and b[2].out_channels == 64 and b[2].bias is not None):
                return 0
            if not _light_closing(c):
                return 0
            mid, ct = c[-2][1].conv, c[-1]
            if not (mid.out_channels == 80 and 72 <= mid.in_channels <= 96 and mid.in_channels % 8 == 0 and ct.in_channels == 80
                    and ct.out_channels == self.nc and ct.bias is not None):
                return 0
        return fuse

    def _forward_fused(self, xs, nms, fuse, pred, smap, branch=""):
        """forward(nms=...) with head_fuse = 1 / 2: the towers stop one conv (box) / two convs (class) early, their features go to the decode
        kernel with the packed weights of what was skipped.  Returns (Candidates, [None] * levels): the raw maps are not produced."""
        B, dev, dt = xs[0].shape[0], xs[0].device, xs[0].dtype
        cv2, cv3 = getattr(self, branch + "cv2"), getattr(self, branch + "cv3")
        bfeat = [L.empty_nhwc(B, 64, t.shape[2], t.shape[3], dt, dev) for t in xs]
        cbuf = [L.empty_nhwc(B, cv3[i][-2][1].conv.in_channels if fuse == 2 else self.nc, t.shape[2], t.shape[3], dt, dev) for i, t in enumerate(xs)]

        def box_tower(i, t):
            cv2[i][1](cv2[i][0](t), out=bfeat[i])

        def cls_tower(i, t):
            if fuse == 1:
                self._cls_tower(i, t, None, cbuf[i], branch)
            else:
                self._cls_stem(i, t, True, branch, cbuf[i])

        self._run_towers([(2 * i + k, partial(tower, i, t)) for i, t in enumerate(xs) for k, tower in enumerate((box_tower, cls_tower))], smap, dev)
        levels, tails = self._levels(list(zip(bfeat, cbuf)), branch), []
        for i, lv in enumerate(levels):
            bt = self._tail("cv2", i, branch)
            wp, bias, _, _ = ops.packed_conv1x1(bt, lv.box, bt.folded)
            chain = None
            if fuse == 2:
                ct = self._tail("cv3", i, branch)
                chain = ops.pw_chain_packed(ct, lv.cls, cv3[i][-2][1].folded, ct.folded)
                chain = chain[:4] if chain else (None,) * 4  # (a pair outside the chained kernel: the separate launches below)
            tails.append((wp, bias, chain))
        classes = nms.get("classes")
        mask = self._class_mask(classes, dev)
        keep = pred if nms.get("keep_pred") else None
        cand = None
        if all(tl[1] is not None and (tl[2] is None or all(w is not None for w in tl[2])) for tl in tails):  # (weights and every bias present: the kernel's gate)
            cand = ops.head_tail_decode_levels(levels, tails, keep, (nms["conf"], mask, classes, self.nc))
        if cand is None:  # outside the fused kernel after all (a misaligned view): the skipped convs as launches of their own, then today's decode
            plain = []
            for i, lv in enumerate(levels):
                box, cls = self._split(_padded(lv.box, self.no))
                self._tail("cv2", i, branch).run(lv.box, box)
                if fuse == 1:
                    cls = lv.cls
                else:
                    self._cls_close(i, lv.cls, cls, True, branch)
                plain.append(lv._replace(box=box, cls=cls))
            cand = ops.head_decode_levels(plain, keep, nms=(nms["conf"], mask, classes))
        return cand, [None] * len(xs)

    # ---- end2end (NMS-free) inference, reference head.py:93-115 (Detect) / :273-298 (GF2Detect)
    one2many_in_inference = False  # the reference also runs the one2many towers in eval mode and returns their maps next to the result,
    #                                where nothing reads them; True reproduces that ("one2many" is None otherwise)

    def _tower_maps(self, xs, branch):
        """Both towers of every level of one branch, on the caller's stream -> (raw maps, levels)."""
        raws = [_padded(t, self.no) for t in xs]
        for i, t in enumerate(xs):
            self._towers(i, t, raws[i], branch)
        return raws, self._levels([self._split(raw) for raw in raws], branch)

    def _forward_end2end(self, x, xs):
        """-> (y (B, min(max_det, A), 6) fp32 rows [x1,y1,x2,y2,score,class], {"one2many": maps or None, "one2one": maps}): the one2one
        towers, the decode with x1y1x2y2 boxes (decode_bboxes: xywh and not end2end, head.py:163-165) and Detect.postprocess (:167-189)
        as the top-k selection kernel -- no NMS follows (utils/ops.py:224-228 only filters these rows)."""
        if len(xs) > 4:
            raise NotImplementedError("end2end heads: at most 4 pyramid levels")
        raws, levels = self._tower_maps(xs, "one2one_")
        A = sum(t.shape[2] * t.shape[3] for t in xs)
        pred = torch.empty((xs[0].shape[0], 4 + self.nc, A), dtype=torch.float32, device=xs[0].device)
        ops.head_decode_levels(levels, pred, xyxy=True)
        y = ops.e2e_topk(pred, min(self.max_det, A))
        many = self._tower_maps(xs, "")[0] if self.one2many_in_inference else None
        return y if self.export else (y, {"one2many": many, "one2one": raws})

    def _decode(self, levels, pred):
        # every level is decoded by ONE launch (reference: Detect._inference runs after all towers, head.py:84-90,117-148)
        if len(levels) <= 4:
            ops.head_decode_levels(levels, pred)
        else:
            for box, cls, st, q, off in levels:
                ops.head_decode(box, cls, st, q, pred, off)
        return pred

    def decode(self, levels):
        """second half of forward() for callers that deferred it (`defer_decode`): levels -> pred (B, 4+nc, A) fp32."""
        box0 = levels[0][0]
        A = sum(lv[0].shape[2] * lv[0].shape[3] for lv in levels)
        pred = torch.empty((box0.shape[0], 4 + self.nc, A), dtype=torch.float32, device=box0.device)
        return self._decode(levels, pred)

    def bias_init(self):
        """reference head.py:150-161 (needs self.stride); end2end heads also their one2one towers (:158-161)."""
        for br in ("", "one2one_") if self.end2end else ("",):
            for a, b, s in zip(getattr(self, br + "cv2"), getattr(self, br + "cv3"), self.stride):
                a[-1].bias.data[:] = 1.0
                b[-1].bias.data[: self.nc] = math.log(5 / self.nc / (640 / float(s)) ** 2)
        self._reset_caches()

    # ---- one more tower per level (`cv4` of Segment / OBB / Pose)
    def _cv4_tower(self, i, t, out):
        c = self.cv4[i]
        self._tail("cv4", i).run(c[1](c[0](t)), out)

    def _cv4_maps(self, xs, c, tower=None):
        """-> one map per level [(B,c,H_l,W_l) NHWC, pixel stride padded to a multiple of 8 channels] that `tower` (default: cv4[i] as it
        stands) has written, all on the caller's stream."""
        maps = [_padded(t, c) for t in xs]
        for i, t in enumerate(xs):
            (tower or self._cv4_tower)(i, t, maps[i])
        return maps


class Segment(Detect):
    """YOLO Segment head (reference head.py:347-369): Detect plus the mask prototypes `proto` (block.py:112-129) and one coefficient tower
    `cv4` per pyramid level.  Boxes and classes run through Detect.forward unchanged (fused decode and NMS candidates included); the
    coefficient towers write one NHWC map per level, which ey_process_mask reads by anchor index -- nothing is concatenated on the
    predict path."""

    def __init__(self, nc=80, nm=32, npr=256, ch=()):
        super().__init__(nc, ch)
        self.nm = nm
        self.npr = npr
        self.proto = Proto(ch[0], self.npr, self.nm)
        self.cv4 = _plain_towers(ch, max(ch[0] // 4, self.nm), self.nm)

    def mask_maps(self, xs):
        """-> (per-level coefficient maps [(B,nm,H_l,W_l) NHWC], p (B,nm,mh,mw) NHWC), all on the caller's stream."""
        p = self.proto(xs[0])
        return self._cv4_maps(xs, self.nm), p

    def forward(self, x, nms=None):
        """nms=None: the reference's eval-mode return (head.py:360-369): (cat([y, mc], 1) (B,4+nc+nm,A) fp32, (raw maps, mc (B,nm,A), p)).
        nms=dict(...) (predict pipelines, see Detect.forward): (Candidates, (raw maps, [coefficient map per level], p))."""
        self._refuse("Segment")
        xs = [L.as_nhwc(t) for t in x]
        mcs, p = self.mask_maps(xs)
        got = Detect.forward(self, list(xs), nms=nms)
        if nms is not None:
            if getattr(self, "defer_decode", False):
                raise NotImplementedError("Segment: pipelined (deferred) decode is not built for the segment task")
            cand, raw = got
            return cand, (raw, mcs, p)
        y, raw = got
        mc = torch.cat([m.flatten(2) for m in mcs], 2)  # (layout only: the reference's view + cat, head.py:365)
        return torch.cat([y, mc.to(y.dtype)], 1), (raw, mc, p)


class WorldDetect(Detect):
    """YOLO-World head (reference head.py:479-521): Detect whose class tower ends in an `embed`-channel map that a contrastive head `cv4`
    (BNContrastiveHead, block.py:670-692) compares with the text embeddings.  For a fixed vocabulary of n texts that tail is affine in the
    tower's hidden map h:
        logits = s W^ (A (W3 h + b3) + d) + beta = (s W^ A W3) h + (s W^ (A b3 + d) + beta)
    with W^ the row-normalised text matrix, A / d the eval-mode BatchNorm's scale / shift, s = exp(logit_scale), beta the head bias.  The
    (n x c3) weight and the bias are computed per level in float64 on the host, once per vocabulary, and run as the class tower's closing 1x1
    conv: from there on this is a Detect head with nc = n, decode and NMS candidate kernels unchanged.  `set_text` supplies the vocabulary;
    `nc` and `no` follow it.  with_bn=False (ContrastiveHead: a per-pixel L2 norm, not affine) is not built."""

    max_vocab = 252  # classes the head-decode kernel's LDS tile takes in fp32 storage (ey_head_decode_levels: 128 anchors x (64 + nc) logits in 160 KiB)

    def __init__(self, nc=80, embed=512, with_bn=False, ch=()):
        super().__init__(nc, ch)
        if not with_bn:
            raise NotImplementedError("WorldDetect(with_bn=False): ContrastiveHead (per-pixel L2 normalisation, yolov8-world.yaml) is not built; "
                                      "the worldv2 YAML uses with_bn=True")
        from .block import BNContrastiveHead
        self.embed = embed
        self.cv3 = _plain_towers(ch, max(ch[0], min(self.nc, 100)), embed)
        self.cv4 = nn.ModuleList(BNContrastiveHead(embed) for _ in ch)
        self.__dict__["_txt"] = None

    def set_text(self, txt):
        """txt: (1, n, embed) text embeddings (the model's original text, not one an ImagePoolingAttn refined); sets nc / no and drops the folds
        (the class-filter masks are keyed by nc)."""
        if txt.dim() != 3 or txt.shape[0] != 1 or txt.shape[2] != self.embed:
            raise ValueError(f"WorldDetect: text must be (1, n, {self.embed}), got {tuple(txt.shape)}")
        n = int(txt.shape[1])
        if not 1 <= n <= self.max_vocab:
            raise NotImplementedError(f"WorldDetect: a vocabulary of {n} texts; the head decode and NMS kernels take 1 to {self.max_vocab} classes")
        self.__dict__["_txt"] = txt
        self.nc = n
        self.no = n + self.reg_max * 4
        self._reset_caches()

    def folded_tail(self, i):
        """fp32 (weight (n, c3, 1, 1), bias (n,)) of level i's class tail folded over the current vocabulary (float64 arithmetic)."""
        txt = self.__dict__.get("_txt")
        if txt is None:
            raise RuntimeError("WorldDetect: no text set (WorldModel.set_classes / set_text supply it)")
        conv, head = self.cv3[i][2], self.cv4[i]
        bn = head.norm
        dev = conv.weight.device
        f = lambda t: t.detach().to(dev).double()  # noqa: E731
        w3, b3 = f(conv.weight).flatten(1), f(conv.bias)
        a = f(bn.weight) / torch.sqrt(f(bn.running_var) + bn.eps)
        d = f(bn.bias) - f(bn.running_mean) * a
        wn = nn.functional.normalize(f(txt)[0], dim=-1, p=2)
        s = torch.exp(f(head.logit_scale))
        w = s * ((wn * a) @ w3)
        b = s * (wn @ (a * b3 + d)) + f(head.bias)
        return w.float().view(*w.shape, 1, 1), b.float()

    def _fold(self, i):
        t = self._tails.get(("fold", i))
        if t is None:
            t = self._tails[("fold", i)] = _Packed()
        return t

    def _cls_tower(self, i, x, raw, out=None, branch=""):
        """class logits of the current vocabulary -> raw[:, 64:] (or `out`): two 3x3 convs, then the folded tail as a 1x1 conv."""
        c = self.cv3[i]
        ops.conv2d(self._fold(i), [c[1](c[0](x))], lambda: self.folded_tail(i), 1, 1, 0, L.ACT_NONE, out=self._split(raw)[1] if out is None else out)

    def forward(self, x, nms=None, towers_only=False):
        if self.__dict__.get("_txt") is None:
            raise RuntimeError("WorldDetect: no text set (WorldModel.set_classes / set_text supply it)")
        if self.end2end:
            raise NotImplementedError("WorldDetect: end2end heads are not built")
        return super().forward(x, nms=nms, towers_only=towers_only)

    def bias_init(self):
        """reference head.py:523-530: only the box towers' biases (the class logits' offset is the contrastive head's bias)."""
        for a in self.cv2:
            a[-1].bias.data[:] = 1.0
        self._reset_caches()


class OBB(Detect):
    """YOLO OBB head (reference head.py:372-399): Detect plus one angle tower `cv4` per pyramid level (`ne` = 1 output channel).  The box and
    class towers run through Detect.forward(towers_only=True); the angle towers write one NHWC map per level; ey_obb_decode_levels then decodes
    all levels in one launch (DFL expectation, dist2rbox with the anchor's angle, class sigmoids, the angle row)."""

    def __init__(self, nc=80, ne=1, ch=()):
        super().__init__(nc, ch)
        self.ne = ne
        self.cv4 = _plain_towers(ch, max(ch[0] // 4, self.ne), self.ne)

    def angle_maps(self, xs):
        """-> per-level angle logit maps [(B,ne,H_l,W_l) NHWC, pixel stride padded to 8 channels], on the caller's stream."""
        return self._cv4_maps(xs, self.ne)

    def forward(self, x, nms=None):
        """The reference's eval-mode return (head.py:383-395): (cat([y, angle], 1) (B,4+nc+1,A) fp32, (raw maps, angle (B,1,A))) with
        angle = (sigmoid(logit) - 0.25) * pi; rows 0-3 of y are the rotated box (cx, cy, w, h) in input pixels."""
        self._refuse("OBB")
        if self.ne != 1:
            raise NotImplementedError(f"OBB: ne={self.ne} (the decode kernel is built for one angle channel)")
        if nms is not None:
            raise NotImplementedError("OBB: the fused NMS candidate build is axis-aligned; run utils.ops.nms_device(pred, rotated=True) on the prediction")
        xs = [L.as_nhwc(t) for t in x]
        angs = self.angle_maps(xs)
        levels, raw = Detect.forward(self, list(xs), towers_only=True)
        B, A = xs[0].shape[0], sum(t.shape[2] * t.shape[3] for t in xs)
        pred = torch.empty((B, 4 + self.nc + 1, A), dtype=torch.float32, device=xs[0].device)
        ops.obb_decode_levels([(lv.box, lv.cls, ang, lv.stride, lv.a_off) for lv, ang in zip(levels, angs)], pred)
        return pred if self.export else (pred, (raw, pred[:, 4 + self.nc:]))


class Pose(Detect):
    """YOLO Pose head (reference head.py:402-451): Detect plus one keypoint tower `cv4` per pyramid level (`nk` = nkpt * ndim channels).
    Boxes and classes run through Detect.forward unchanged (fused decode and NMS candidates included); the keypoint towers write one NHWC
    map per level.  Predict and validation decode the keypoints of the rows NMS kept (ey_kpts_decode_rows reads the maps by anchor index);
    the reference's eval-mode return decodes every anchor with one ey_kpts_decode_levels launch."""

    def __init__(self, nc=80, kpt_shape=(17, 3), ch=()):
        super().__init__(nc, ch)
        self.kpt_shape = kpt_shape  # number of keypoints, number of dims (2 for x,y or 3 for x,y,visible)
        self.nk = kpt_shape[0] * kpt_shape[1]
        self.cv4 = _plain_towers(ch, max(ch[0] // 4, self.nk), self.nk)

    def kpt_maps(self, xs):
        """-> per-level keypoint logit maps [(B,nk,H_l,W_l) NHWC, pixel stride padded to a multiple of 8 channels], on the caller's stream."""
        return self._cv4_maps(xs, self.nk, self._kpt_tower)

    def _kpt_tower(self, i, t, out):
        """Conv(x, c4, 3) -> Conv(c4, c4, 3) -> nn.Conv2d(c4, nk, 1) with c4 = max(x // 4, nk).  The MFMA conv reads sources whose channel
        count is a multiple of 8; c4 = 51 is not, and the second and third conv would take the generic direct kernel (measured 8.8 ms
        instead of 0.06 ms for the 80x80 level at batch 32).  So the tower runs on c4 rounded up to a multiple of 8: the weights are
        packed with zero rows / zero input columns for the extra channels, which therefore hold SiLU(0) = 0 and add 0 to every sum."""
        c = self.cv4[i]
        c4 = c[0].conv.out_channels
        pad = -c4 % 8
        plain = all(isinstance(m, Conv) and m.conv.kernel_size == (3, 3) and m.conv.stride == (1, 1) and m.conv.padding == (1, 1) and m.conv.groups == 1
                    and m.conv.dilation == (1, 1) for m in (c[0], c[1]))
        if not pad or not plain or c[2].kernel_size != (1, 1) or c[2].groups != 1:
            return self._cv4_tower(i, t, out)
        F = nn.functional

        def padded(fn, po, pi):  # (w (O,I,k,k), b (O,)) -> po zero output channels, pi zero input channels appended
            w, b = fn()
            return F.pad(w, (0, 0, 0, 0, 0, pi, 0, po)), F.pad(b, (0, po))

        tail = self._tail("cv4", i)
        h = ops.conv2d(c[0], [t], lambda: padded(c[0].folded, pad, 0), 3, 1, 1, _act_code(c[0].act), tag="kpad")
        h = ops.conv2d(c[1], [h], lambda: padded(c[1].folded, pad, pad), 3, 1, 1, _act_code(c[1].act), tag="kpad")
        return ops.conv2d(tail, [h], lambda: padded(tail.folded, 0, pad), 1, 1, 0, L.ACT_NONE, out=out, tag="kpad")

    def kpt_levels(self, maps):
        """the keypoint maps as the level list of _ops.kpts_decode_levels / kpts_decode_rows: [(map, stride, first anchor)]."""
        return [(m, st, off) for m, (st, off) in zip(maps, self._walk(maps))]

    decode_kpts = True  # instance attribute (or forward keyword): False leaves the (B,nk,A) decode out of the nms=None return, see forward

    def forward(self, x, nms=None, decode_kpts=None):
        """nms=None: the reference's eval-mode return (head.py:414-422): (cat([y, pred_kpt], 1) (B,4+nc+nk,A) fp32, (raw maps, kpt (B,nk,A)
        logits)); the keypoint rows are decoded straight into the prediction tensor.  decode_kpts=False (validation; keyword, or the head
        attribute of that name): (y (B,4+nc,A), (raw maps, [keypoint map per level])) -- the (B,nk,A) decode is left out,
        ey_kpts_decode_rows serves the kept rows.
        nms=dict(...) (predict pipelines, see Detect.forward): (Candidates, (raw maps, [keypoint map per level]))."""
        self._refuse("Pose")
        if self.kpt_shape[1] not in (2, 3) or self.nk > 256 or len(x) > 4:
            raise NotImplementedError(f"Pose: kpt_shape={tuple(self.kpt_shape)} on {len(x)} levels (the keypoint kernels are built for ndim 2 or 3, nk <= 256, <= 4 levels)")
        if getattr(self, "defer_decode", False):
            raise NotImplementedError("Pose: pipelined (deferred) decode is not built for the pose task")
        xs = [L.as_nhwc(t) for t in x]
        maps = self.kpt_maps(xs)
        if nms is not None:
            cand, raw = Detect.forward(self, list(xs), nms=nms)
            return cand, (raw, maps)
        if not (self.decode_kpts if decode_kpts is None else decode_kpts):
            y, raw = Detect.forward(self, list(xs))
            return y, (raw, maps)
        levels, raw = Detect.forward(self, list(xs), towers_only=True)
        B, A, no = xs[0].shape[0], sum(t.shape[2] * t.shape[3] for t in xs), 4 + self.nc
        pred = torch.empty((B, no + self.nk, A), dtype=torch.float32, device=xs[0].device)
        if B == 1:  # the box / class rows of one image are contiguous: the Detect decode writes them in place
            self._decode(levels, pred[:, :no])
        else:
            pred[:, :no].copy_(self._decode(levels, torch.empty((B, no, A), dtype=torch.float32, device=pred.device)))
        ops.kpts_decode_levels(self.kpt_levels(maps), self.kpt_shape, pred[:, no:])
        kpt = torch.cat([m.flatten(2) for m in maps], 2)  # (layout only: the reference's view + cat of the logits, head.py:417)
        return pred if self.export else (pred, (raw, kpt))


class GF2Detect(Detect):
    """GFLv2-style quality head on top of Detect (reference head.py:194-345): q = DGQP(softmax(box logits)),
    score = sigmoid(cls) * clamp(q, 1e-6, 1-1e-6)."""

    def __init__(self, nc=80, ch=()):
        super().__init__(nc, ch)
        self.reg_topk = 4
        self.add_mean = True
        self.reg_channels = 64
        self.apply_quality_in_inference = True
        self.reg_conf = _reg_conf(ch, self.reg_topk, self.add_mean, self.reg_channels)
        if self.end2end:  # head.py:220-221
            self.one2one_reg_conf = copy.deepcopy(self.reg_conf)
        self._qcache = {}

    def _quality_params(self, i, device, branch=""):
        if not self.apply_quality_in_inference:
            return None
        if self.reg_topk != 4 or not self.add_mean:
            raise NotImplementedError("the decode kernel is built for reg_topk=4, add_mean=True (the reference defaults)")
        q = self._qcache.get((branch, i, device))
        if q is None:
            m = getattr(self, branch + "reg_conf")[i]
            f = lambda t: t.detach().float().to(device).contiguous()  # noqa: E731
            q = self._qcache[(branch, i, device)] = (f(m[0].weight).view(m[0].out_channels, -1), f(m[0].bias), f(m[2].weight).view(-1), f(m[2].bias))
        return q


class E2EDetect(GF2Detect):
    """NMS-free head (reference head.py:799-824): GF2Detect with end2end = True -- one2one copies of both towers and of the quality
    head (:76-78,220-221), decoded as x1y1x2y2 and reduced to the max_det best rows by Detect.postprocess (:167-189, :273-298).  The
    class tower is the depthwise structure whatever `legacy` says (:812-822)."""

    end2end = True

    def __init__(self, nc=80, ch=()):
        super().__init__(nc, ch)
        self.cv3 = _light_towers(ch, max(ch[0], min(self.nc, 100)), self.nc)
        self.one2one_cv3 = copy.deepcopy(self.cv3)


class v10Detect(Detect):
    """YOLOv10 head (reference head.py:764-797): Detect with end2end = True and the light class tower (depthwise 3x3 -> 1x1 -> depthwise 3x3 ->
    1x1 -> nn.Conv2d) whatever `legacy` says; one2one_cv3 is a deep copy of it.  The one2one towers, the x1y1x2y2 decode and the top-k
    selection (ey_e2e_topk) are Detect's end2end path."""

    end2end = True
    legacy = False  # parse_model does not assign it (reference tasks.py:1096): the class default stays visible

    def __init__(self, nc=80, ch=()):
        super().__init__(nc, ch)
        self.cv3 = _light_towers(ch, max(ch[0], min(self.nc, 100)), self.nc)
        self.one2one_cv3 = copy.deepcopy(self.cv3)


class GFLHeadv2_uniH(GF2Detect):
    """reference head.py:827-908.  stem/dat/pos/cit are nn.Identity placeholders there (use_* default False);
    forward == GF2Detect.forward through the `super()` calls at :898,:907."""

    def __init__(self, nc=80, ch=(), reg_topk=4, add_mean=True, reg_channels=64, use_dat=False, use_cit=False, use_poscnn=False):
        super().__init__(nc, ch)
        if use_dat or use_cit or use_poscnn:
            raise NotImplementedError("use_dat/use_cit/use_poscnn only add nn.Identity placeholders in the reference; not built")
        self.stem = nn.ModuleList(nn.Identity() for _ in ch)
        self.dat = self.pos_cls = self.pos_reg = self.cit_cls = self.cit_reg = None
        self.reg_topk = reg_topk
        self.add_mean = add_mean
        self.reg_channels = reg_channels
        self.reg_conf = _reg_conf(ch, self.reg_topk, self.add_mean, self.reg_channels)


class Classify(_Packed):
    """YOLO classification head (reference head.py:454-476): x (B, c1, H, W) -> (probabilities, logits), both (B, c2) fp32.  Same attribute
    names and state_dict keys (conv.conv.weight, conv.bn.*, linear.weight, linear.bias); `pool` and `drop` hold no tensors and are never
    called.  The eval forward is two launches: ey_classify_pool (the 1x1 conv to 1280 channels with the folded BatchNorm, SiLU and the mean
    over the pixels: the 1280-channel map never exists) and ey_classify_linear_softmax (linear, softmax and the top-5 classes).  The top-5
    indices and probabilities of the last forward are kept in `top5` for the validator and `Probs` (fixed-size device tensors)."""

    export = False

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1):
        super().__init__()
        if k != 1 or s != 1 or g != 1:
            raise NotImplementedError(f"Classify(k={k}, s={s}, g={g}): only the 1x1, stride-1, dense conv of the shipped YAMLs is built")
        c_ = 1280  # efficientnet_b0 size
        self.conv = Conv(c1, c_, k, s, p, g)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.drop = nn.Dropout(p=0.0, inplace=True)
        self.linear = nn.Linear(c_, c2)
        self.top5 = None

    def _weights(self, dtype, device):
        def build():
            w, b = self.conv.folded()
            return (w.reshape(w.shape[0], -1).to(device=device, dtype=dtype).contiguous(), b.to(device=device, dtype=torch.float32).contiguous(),
                    self.linear.weight.detach().to(device=device, dtype=dtype).contiguous(), self.linear.bias.detach().to(device=device, dtype=torch.float32).contiguous())
        return self._packed(("cls", dtype, device), build)

    def forward(self, x):
        if self.training:
            raise NotImplementedError("Classify: the training forward (logits only) is outside the built inference path")
        if self.linear.out_features > 8192:
            raise NotImplementedError(f"Classify: nc={self.linear.out_features} (1 to 8192 classes are built)")
        if isinstance(x, list):
            x = ops.concat(x)
        x = ops.as_tensor(x)
        if hasattr(self.conv, "bn") and self.conv.bn.training:
            raise NotImplementedError("Classify: BatchNorm in training mode")
        wc, bc, wl, bl = self._weights(x.dtype, x.device)
        pooled = ops.classify_pool(x, wc, bc, _act_code(self.conv.act))
        logits, probs, topi, topp = ops.classify_linear_softmax(pooled, wl, bl)
        self.top5 = (topi, topp)
        return probs if self.export else (probs, logits)
