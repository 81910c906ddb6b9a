"""-m gpu: the block-program kernels (csrc/block.hip: block_tile_kernel = pointwise chains, on by default; block_kernel = one
workgroup per image, opt-in) against the fp64 graph reference of tests/fp64_ref.py, at every instantiation.

The cases live in tests/block_cases.py (test_block_ref_cpu.py proves without a GPU that their exact data stays exact in f16 through
every stage and that they span the four tile_conv<NTI> and the nine blk_conv<MT,NTI>).  Every case is ordinary wrapper code
(nn._ops.conv2d / dwconv / dsconv / dwt_haar / sppf_pool) run through nn._block.BlockCache; the traced label is asserted, so a silent
fallback to the per-layer kernels fails, and the compiled stages are read back from the device image of the program to assert the
instantiation (tile_nti, or mt x nti) and the LDS placement of every source / residual / output of a tiled chain.

* exact: bit-identical to fp64 (fp64_ref.assert_exact); inputs are channel slices of NaN-filled buffers, outputs slices of
  sentinel-filled ones; single-tap probes name a row mix-up by position.
* bounded: general data, SiLU in place of ReLU, per-element bound of graph_ref and the mean-ulp gate of fp64_ref.report.
* the real chains of C2PSA_LinearAttention with the module's folded weights.
* recording / replay: other addresses, other data, caller-supplied and fresh outputs, another offset inside the storage.
* BLOCK_COVERED: the block labels of the benchmarked step (asserted by test_gpu_conv_exact.py, which replays each chain here)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import block_cases as BC  # noqa: E402
import fp64_ref as R  # noqa: E402
import test_gpu_conv_exact as CE  # noqa: E402
from gpu_util import _traced, load_synth, to_dev  # noqa: E402

F16 = torch.float16
# block labels of the step -> the test here that holds the kernel to fp64 at the step's own shapes
BLOCK_COVERED = {
    "block_tile_kernel<C2PSA_LinearAttention.proj_ffn_cv2>": "test_c2psa_chains_within_fp64_bound, test_gpu_conv_exact.py::test_step_block_chains_replay_exact",
    "block_tile_kernel<C2PSA_LinearAttention.cv1_qkv>": "test_c2psa_chains_within_fp64_bound",
}
_SEEN_NTI, _SEEN_TILES, _SEEN_OPS, _DONE = set(), set(), set(), set()


def compiled(prog):
    """the compiled stages (nn._lib.BlockStage) read back from the device image of a program"""
    from edge_yolo_amd import _lib as L
    return list((L.BlockStage * prog.n).from_buffer_copy(prog.prog.cpu().numpy().tobytes()))


class Run:
    """One case as a BlockCache: data, device tensors, the chain in wrapper code, the checks."""

    def __init__(self, case, general=False, tag=None):
        from edge_yolo_amd.nn import _block
        self.c, self.general = case, general
        self.inputs, self.wts, self.nodes = BC.make(case, general)
        self.sh = BC.shapes(case)
        self.keys = list(case["inputs"])
        self.holders = {nd["out"]: CE._holder() for nd in case["nodes"]}
        self.tag = tag or case["name"]
        self.cache = _block.BlockCache(self.tag, tiled=case["tiled"])
        self.label = f"{'block_tile_kernel' if case['tiled'] else 'block_kernel'}<{self.tag}>"

    # ---- tensors
    def dev_inputs(self, inputs=None, shifted=False):
        """device views in key order; padded inputs are the channels [8, 8 + C) of a NaN buffer ([0, C) when shifted)"""
        from edge_yolo_amd import _lib as L
        inputs = inputs or self.inputs
        out = []
        for key in self.keys:
            v = self.c["inputs"][key]
            C, h, w = self.sh[key]
            if shifted and v["pad"]:
                buf = L.empty_nhwc(self.c["B"], C + v["pad"], h, w, F16, "cuda")
                buf.fill_(float("nan"))
                t = buf[:, :C]
                t.copy_(inputs[key])
                out.append(t)
            else:
                out.append(CE._nhwc(self.c["B"], C, h, w, F16, inputs[key], v["pad"]))
        return out

    def out_views(self):
        """{output key: (buffer, view)}: sentinel-filled buffers for the outputs the case writes as channel slices"""
        from edge_yolo_amd import _lib as L
        res = {}
        for key in self.c["outs"]:
            C, h, w = self.sh[key]
            lay = self.c.get("out_layout", {}).get(key) or ((C + 24, 16) if key in self.c["out_slice"] else None)
            if lay is not None:
                buf = L.empty_nhwc(self.c["B"], lay[0], h, w, F16, "cuda")
                buf.fill_(5.0)
                res[key] = (buf, buf[:, lay[1]:lay[1] + C])
        return res

    # ---- the chain in ordinary wrapper code
    def fn(self, outviews=None):
        from edge_yolo_amd import _lib as L
        from edge_yolo_amd.nn import _ops
        c, B = self.c, self.c["B"]
        ov = {k: v[1] for k, v in (outviews or {}).items()}

        def run(*ins):
            env = dict(zip(self.keys, ins))

            def src(spec):
                if spec is None:
                    return None
                return env[spec] if isinstance(spec, str) else env[spec[0]][:, spec[1]:spec[2]]
            for nd in c["nodes"]:
                o, wt, out, hold = nd["out"], self.wts.get(nd["out"]), ov.get(nd["out"]), self.holders[nd["out"]]
                C, h, w = self.sh[o]
                if nd["op"] == "conv":
                    sets, ng, co, k = wt["sets"], nd["ngroup"], nd["cout"], nd["k"]
                    if nd["into"] is not None:
                        out = env[nd["into"][0]][:, nd["into"][1]:nd["into"][1] + co]
                    srcs, res, z, kw = [src(s) for s in nd["srcs"]], src(nd["res"]), src(nd["addz"]), {}
                    wfn = (lambda sets=sets: (sets[0][0].float(), sets[0][1]))
                    if ng > 1:
                        full = out if out is not None else L.empty_nhwc(B, ng * co, h, w, F16, "cuda")
                        cin = srcs[0].shape[1] // ng
                        kw = dict(ngroup=ng, src_gstride=cin, y_gstride=co, w_sets=nd["w_sets"])
                        srcs, out = [srcs[0][:, :cin]], full[:, :co]
                        res, z = (res[:, :co] if res is not None else None), (z[:, :co] if z is not None else None)
                        if nd["w_sets"] > 1:
                            wfn = (lambda sets=sets: [(w_.float(), b_) for w_, b_ in sets])
                    y = _ops.conv2d(hold, srcs, wfn, k, nd["s"], k // 2, wt["act"], out=out, res=res, addz=z, out_scale=nd["out_scale"], **kw)
                    env[o] = full if ng > 1 else y
                elif nd["op"] == "dw":
                    env[o] = _ops.dwconv(hold, src(nd["srcs"][0]), lambda wt=wt: (wt["w"].float(), wt["b"]), nd["k"], wt["act"], out=out)
                elif nd["op"] == "ds":
                    y = _ops.dsconv(hold, src(nd["srcs"][0]), lambda wt=wt: (wt["wd"].float(), wt["bd"].float()), lambda wt=wt: (wt["wp"].float(), wt["bp"]),
                                    nd["k"], wt["act"], out=out, res=src(nd["res"]))
                    assert y is not None, "dsconv refused the shape"
                    env[o] = y
                elif nd["op"] == "dwt":
                    env[o] = _ops.dwt_haar(src(nd["srcs"][0]), out=out)
                else:
                    x = src(nd["srcs"][0])
                    full = out if out is not None else L.empty_nhwc(B, C, h, w, F16, "cuda")
                    ci = C // 3
                    _ops.sppf_pool(x, full[:, :ci], full[:, ci:2 * ci], full[:, 2 * ci:])
                    env[o] = full
            return [env[k] for k in c["outs"]]
        return run

    # ---- launch + checks
    def launch(self, ins, outviews=None, pass_outs=False):
        outs = [outviews[k][1] for k in self.c["outs"]] if pass_outs else None
        got, labels = _traced(lambda: self.cache.run(self.fn(outviews), ins, outs))
        assert got is not None, f"{self.c['name']}: not block-executable (the per-layer kernels would have run instead)"
        assert labels == [self.label], f"{self.c['name']}: launched {labels}, expected one {self.label}"
        return got

    def check_program(self):
        """the compiled stages carry the instantiation the mirrors predict and, tiled, the LDS placement the case is meant for"""
        from edge_yolo_amd import _lib as L
        c = self.c
        st = compiled(self.cache.progs[-1])
        convs = [s for s in st if s.op == L.BLK_CONV]
        exp = BC.expected_tiles(c)
        assert len(convs) == len(exp)
        got = [s.tile_nti if c["tiled"] else (s.mt, s.nti) for s in convs]
        assert got == exp, f"{c['name']}: compiled tiles {got}, the host-side mirror of ey_block_compile says {exp}"
        assert c["want"] <= set(got), f"{c['name']}: meant to exercise {sorted(c['want'])}, runs {got}"
        (_SEEN_NTI if c["tiled"] else _SEEN_TILES).update(got)
        _SEEN_OPS.update(s.op for s in st)
        if c["tiled"]:
            assert len(st) == len(c["nodes"])
            for s, nd in zip(st, c["nodes"]):
                for j, sp in enumerate(nd["srcs"]):
                    assert (s.tile_src_lds[j] >= 0) == BC.lds_resident(c, BC._key(sp)), f"{c['name']} stage {nd['out']}: source {j} placement"
                    if not isinstance(sp, str) and BC.lds_resident(c, sp[0]):  # a channel slice of an LDS tensor: offset inside its row
                        base = next(q.tile_y_lds for q, n2 in zip(st, c["nodes"]) if n2["out"] == sp[0])
                        assert s.tile_src_lds[j] == base + sp[1], f"{c['name']} stage {nd['out']}: LDS slice offset"
                assert (s.tile_y_lds >= 0) == BC.lds_resident(c, nd["out"]), f"{c['name']} stage {nd['out']}: output placement"
                if nd["res"] is not None:
                    assert s.has_res and (s.tile_res_lds >= 0) == BC.lds_resident(c, BC._key(nd["res"])), f"{c['name']} stage {nd['out']}: res placement"
        return st

    def reference(self, inputs=None):
        exact = not self.general

        def on_node(nd, y, bnd):
            if exact:
                assert torch.equal(y.to(F16).double(), y), f"{self.c['name']}: stage {nd['out']} of the reference is not exact in f16"
        return R.graph_ref({k: v.cuda() for k, v in (inputs or self.inputs).items()}, self.nodes, on_node=on_node)

    def check(self, got, ins, outviews, inputs=None, what="", mean_ulp_max=0.5):
        """outputs (and the channels of inputs written in place) against fp64: bit for bit, or within the graph bound"""
        c = self.c
        ref = self.reference(inputs)
        name = f"{c['name']}{what}"
        pairs = [(k, g) for k, g in zip(c["outs"], got)]
        for key, lo, stage in c["check_inputs"]:
            t = ins[self.keys.index(key)]
            pairs.append((stage, t[:, lo:lo + ref[stage][0].shape[1]]))
        stats = {}
        for k, g in pairs:
            y, bnd = ref[k]
            assert tuple(g.shape) == tuple(y.shape), (name, k, tuple(g.shape), tuple(y.shape))
            if self.general:
                stats[k] = R.report(f"{name} {k}", self.label, g, y, bnd, mean_ulp_max)
            else:
                R.assert_exact(f"{name} {k}", self.label, g, y)
        for key, (buf, view) in (outviews or {}).items():
            C = view.shape[1]
            lo = (view.data_ptr() - buf.data_ptr()) // 2
            keep = torch.cat([buf[:, :lo], buf[:, lo + C:]], 1)
            assert bool((keep == 5.0).all()), f"{name}: {key} written outside its output channel slice"
        return stats


def _per_layer_mean_ulp(r):
    """mean ulp of the same wrapper code run one launch per stage (the stand-alone kernels, each held to fp64 by its own test file)
    against the same reference on the same inputs"""
    ins = r.dev_inputs()
    got, labels = _traced(lambda: r.fn()(*ins))
    assert not any(lab.startswith("block_") for lab in labels), labels
    ref = r.reference()
    return max(R.report(f"{r.c['name']} per-layer {k}", "per-layer", g, ref[k][0], ref[k][1], float("inf"))[1] for k, g in zip(r.c["outs"], got))


def _go(case, general=False):
    r = Run(case, general)
    ins, ov = r.dev_inputs(), r.out_views()
    got = r.launch(ins, ov)
    r.check_program()
    gate = 0.5
    if general and len(case["nodes"]) > 4 and not case["tiled"]:
        # The 0.5-ulp gate describes ONE rounding.  In a deep per-image program every f16 intermediate that rounds to the other
        # neighbour (both roundings are within that stage's bound) is spread by the pool chain over up to 13 x 13 pixels and summed by
        # the last conv over hundreds of channels, so the mean error of the end result is not tied to half an ulp even for exact
        # arithmetic per stage.  The per-element bound is the check; the mean gate is what the issue prescribes for chains:
        # 1.25 x the mean ulp of the one-launch-per-stage form measured here, on the same inputs, against the same reference.
        mu = _per_layer_mean_ulp(r)
        gate = max(0.5, 1.25 * mu)
        print(f"[gate] {case['name']}: per-layer form mean ulp {mu:.3f} -> gate {gate:.3f}")
    r.check(got, ins, ov, what=" silu" if general else "", mean_ulp_max=gate)
    if not general:
        _DONE.add(case["name"])
    return r


# ------------------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("name", [c["name"] for c in BC.TILE_CASES])
def test_tile_kernel_exact(name):
    """block_tile_kernel: every tile_conv<NTI>, channel / pixel tails, source / residual / output placements, addz, in-place tail"""
    _go(BC.BY_NAME[name])


@pytest.mark.parametrize("name", [c["name"] for c in BC.BLOCK_CASES])
def test_block_kernel_exact(name):
    """block_kernel: the nine blk_conv<MT,NTI> (groups with res / addz, strides, Cin tails, k-loop tails), blk_dw, the DSConv
    recording, blk_dwt, blk_pool (max is exact for any data: general, all-negative, +-inf), a mixed program end to end"""
    _go(BC.BY_NAME[name])


@pytest.mark.parametrize("name", [c["name"] for c in BC.TILE_REFUSED])
def test_tile_kernel_refuses_and_caller_keeps_per_conv_result(name):
    """9 stages (TILE_MAX_STAGES = 8) or more than 56 KB of LDS: BlockCache.run returns None, nothing is launched, and the same
    wrapper code run by the caller (one launch per conv, the kernels test_gpu_conv_exact.py holds to fp64) gives the exact result"""
    c = BC.BY_NAME[name]
    r = Run(c)
    ins = r.dev_inputs()
    got, labels = _traced(lambda: r.cache.run(r.fn(), ins))
    assert got is None and labels == [], (got, labels)
    got, labels = _traced(lambda: r.fn()(*ins))
    assert len(labels) == len(c["nodes"]) and all(lab.startswith("conv_") for lab in labels), labels
    ref = r.reference()
    for k, g in zip(c["outs"], got):
        R.assert_exact(f"{name} per-conv {k}", labels[-1], g, ref[k][0])


def test_every_instantiation_ran():
    """the union over the exact matrix above: four tile_conv<NTI>, nine blk_conv<MT,NTI>, every per-image operator"""
    from edge_yolo_amd import _lib as L
    for c in BC.TILE_CASES + BC.BLOCK_CASES:  # (run alone: the cases that have not run in this session)
        if c["name"] not in _DONE:
            _go(c)
    print(f"[coverage] tile_conv NTI {sorted(_SEEN_NTI)}; blk_conv MTxNTI {sorted(_SEEN_TILES)}; block ops {sorted(_SEEN_OPS)}")
    assert _SEEN_NTI == BC.TILE_NTIS, sorted(_SEEN_NTI)
    assert _SEEN_TILES == BC.BLK_TILES, sorted(_SEEN_TILES)
    assert {L.BLK_CONV, L.BLK_DW, L.BLK_DWT, L.BLK_POOL} <= _SEEN_OPS


# ------------------------------------------------------------------------------------------------------------------------ bounded
@pytest.mark.parametrize("name", [c["name"] for c in BC.ALL_CASES if c["bounded"]])
def test_block_kernels_silu_within_fp64_bound(name):
    """general data (f16 inputs / weights, fp32 biases), SiLU in place of ReLU: the per-element bound of the graph reference (every
    stage's own bound plus what its sources, residual and addz inherit) and the mean-ulp gate (0.5).  s_addz_quarter_relu takes the
    SiLU / out_scale == 1 fast branch of blk_epilogue, s_addz_half_scale the general one with SiLU."""
    _go(BC.BY_NAME[name], general=True)


# ------------------------------------------------------------------------------------------------------------------------ C2PSA
def _capture_chains(mh, xd):
    """one forward of the module with the inputs (cloned before the launch) and outputs of every BlockCache.run recorded"""
    from edge_yolo_amd.nn import _block
    seen = []
    orig = _block.BlockCache.run

    def rec(self, fn, ins, outs=None):
        before = [t.clone() for t in ins]
        r = orig(self, fn, ins, outs)
        seen.append((self.tag, before, list(ins), r))
        return r
    _block.BlockCache.run = rec
    try:
        y, labels = _traced(lambda: mh(xd))
    finally:
        _block.BlockCache.run = orig
    return y, labels, seen


def _c2psa_nodes(mh):
    blk, c = mh.m[0], mh.c
    at = blk.attn

    def q(wb):
        w, b = wb
        return w.detach().float().half().double().cpu(), (b.detach().float().cpu() if b is not None else None)
    from edge_yolo_amd.nn.modules.conv import fold_bn
    w1, b1 = q(mh.cv1.folded())
    wq, bq = q(fold_bn(at.qkv.weight, at.qkv.bias, None))
    wp, bp = q((at.proj.weight, at.proj.bias))
    wf0, bf0 = q(blk.ffn[0].folded())
    wf1, bf1 = q(blk.ffn[1].folded())
    w2, b2 = q(mh.cv2.folded())
    head = [R.gnode("t", ["x"], w1, b1, act=R.ACT_SILU), R.gnode("qkv", [("t", c, 2 * c)], wq, bq)]
    tail = [R.gnode("x1", ["y"], wp, bp, res=("t", c, 2 * c)), R.gnode("f", ["x1"], wf0, bf0, act=R.ACT_SILU),
            R.gnode("x2", ["f"], wf1, bf1, res="x1", into=("t", c)), R.gnode("o", ["t"], w2, b2, act=R.ACT_SILU)]
    return head, tail


@pytest.mark.parametrize("c1,B,H,W", [(256, 1, 20, 20), (256, 32, 20, 20), (128, 2, 13, 17), (512, 2, 13, 17)])
def test_c2psa_chains_within_fp64_bound(c1, B, H, W):
    """Both pointwise chains of C2PSA_LinearAttention ([cv1 -> qkv] forced on, and the default [proj -> ffn -> ffn -> cv2]) with the
    module's folded weights and SiLU on general data: each chain's outputs against the graph reference evaluated on the chain's own
    inputs (the tail's x2 read back from the slice of t it overwrote), per-element bound + the 0.5 mean-ulp gate (measured on
    MI355X: chains 0.25 .. 0.36 ulp, the one-launch-per-conv form the same figures).  The one-launch-per-conv form
    (pw_chains = False) runs on the same inputs: chain and per-conv form round at the same points and walk K in the same 32-channel
    steps, and their results are bit-identical (t, x2 and the output; asserted)."""
    from edge_yolo_amd.nn import modules as M
    from edge_yolo_amd import _lib as L
    m = M.C2PSA_LinearAttention(c1, c1, 1)
    load_synth(m, "c2psa")
    mh = to_dev(m, F16)
    c = mh.c
    x = torch.randn((B, c1, H, W), generator=BC.gen("c2psa", c1, B, H, W)).half()
    xd = L.empty_nhwc(B, c1, H, W, F16, "cuda")
    xd.copy_(x)
    mh.pw_chains = True
    y, labels, seen = _capture_chains(mh, xd)
    tags = ["C2PSA_LinearAttention.cv1_qkv", "C2PSA_LinearAttention.proj_ffn_cv2"]
    assert [lab for lab in labels if lab.startswith("block_")] == [f"block_tile_kernel<{t}>" for t in tags] and len(labels) == 3, labels
    assert [s[0] for s in seen] == tags and all(s[3] is not None for s in seen)
    head, tail = _c2psa_nodes(mh)
    case = f"c2psa c{c1} b{B} {H}x{W}"
    # per-conv form on the same inputs
    mh.pw_chains = False
    t_pc = mh.cv1(xd)
    # ---- head: x -> t, qkv
    (_, before, _, res) = seen[0]
    ref = R.graph_ref(dict(x=before[0]), head)
    t_head = seen[1][1][1]  # t as the head left it (the tail has since written x2 over its second half): the tail's input, cloned
    st_h = {k: R.report(f"{case} cv1_qkv {k}", f"block_tile_kernel<{tags[0]}>", g, ref[k][0], ref[k][1]) for k, g in (("t", t_head), ("qkv", res[1]))}
    R.report(f"{case} per-conv cv1 t", "per-conv", t_pc, ref["t"][0], ref["t"][1])
    assert torch.equal(t_head, t_pc), f"{case}: cv1 of the chain differs from the per-conv form"
    # ---- tail: y, t -> x2 (over t[:, c:]), o
    (_, before, live, res) = seen[1]
    ins = dict(y=before[0], t=before[1])
    ref = R.graph_ref(ins, tail)
    lab = f"block_tile_kernel<{tags[1]}>"
    R.report(f"{case} proj_ffn_cv2 x2", lab, live[1][:, c:], ref["x2"][0], ref["x2"][1])
    R.report(f"{case} proj_ffn_cv2 o", lab, res[0], ref["o"][0], ref["o"][1])
    assert res[0].data_ptr() == y.data_ptr()
    # the same tail, one launch per conv, on clones of the same inputs
    blk, at = mh.m[0], mh.m[0].attn
    from edge_yolo_amd.nn import _ops
    y2, t2 = before[0].clone(), before[1].clone()
    x1 = _ops.conv2d(at, [y2], lambda: (at.proj.weight.detach().float(), at.proj.bias.detach().float() if at.proj.bias is not None else None), 1, 1, 0,
                     L.ACT_NONE, res=t2[:, c:], tag="proj")
    blk.ffn[1](blk.ffn[0](x1), out=t2[:, c:], res=x1)
    o2 = mh.cv2(t2)
    torch.cuda.synchronize()
    _, mu_pc = R.report(f"{case} per-conv o", "per-conv", o2, ref["o"][0], ref["o"][1])
    assert torch.equal(live[1][:, c:], t2[:, c:]) and torch.equal(res[0], o2), f"{case}: the tail chain differs from the per-conv form"
    print(f"[c2psa] {case}: chains bit-identical to the per-conv form; head (max err/bound, mean ulp) {st_h}; per-conv tail mean ulp {mu_pc:.3f}")


# ------------------------------------------------------------------------------------------------------------------------ replay
@pytest.mark.parametrize("name", ["c_lds_tails", "x_mixed"])
def test_recorded_program_serves_other_tensors(name):
    """BlockRecorder.finish rebases every pointer into an external tensor to (index, byte offset): a recorded program must read the
    tensors of the CALL.  (a) fresh allocations with other data while the recording's own inputs are overwritten with NaN;
    (b) caller-supplied outputs; (c) outs=None twice -- fresh outputs each time, the first result untouched by the second run;
    (d) inputs at another byte offset of their storage: matches() is false, a second program is recorded, not the first misapplied."""
    c = BC.BY_NAME[name]
    r = Run(c)
    ins0, ov0 = r.dev_inputs(), r.out_views()
    got0 = r.launch(ins0, ov0)
    r.check(got0, ins0, ov0, what=" record")
    prog = r.cache.progs[-1]
    # (a) + (b): other data at other addresses into caller-supplied outputs; the recording's inputs now hold NaN
    in1 = BC.make(c, variant=1)[0]
    ins1, ov1 = r.dev_inputs(in1), r.out_views()
    for t in ins0:
        t.fill_(float("nan"))
    assert prog.matches(ins1) and all(a.data_ptr() != b.data_ptr() for a, b in zip(ins0, ins1))
    got1 = r.launch(ins1, ov1, pass_outs=True)
    assert len(r.cache.progs) == 1 and all(g.data_ptr() == ov1[k][1].data_ptr() for g, k in zip(got1, c["outs"]))
    r.check(got1, ins1, ov1, inputs=in1, what=" replay other data")
    # (c) outs=None twice
    got2 = r.launch(ins1)
    keep2 = [g.clone() for g in got2]
    r.check(got2, ins1, None, inputs=in1, what=" replay fresh outs")
    in3 = BC.make(c, variant=2)[0]
    ins3 = r.dev_inputs(in3)
    got3 = r.launch(ins3)
    torch.cuda.synchronize()
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(got2, got3)), "the second run reused the first run's outputs"
    assert all(torch.equal(a, b) for a, b in zip(got2, keep2)), "the second run changed the first run's result"
    r.check(got3, ins3, None, inputs=in3, what=" replay fresh outs again")
    # (d) another offset inside a storage of the same size
    ins4 = r.dev_inputs(in1, shifted=True)
    assert not prog.matches(ins4)
    got4 = r.launch(ins4)
    assert len(r.cache.progs) == 2
    r.check(got4, ins4, None, inputs=in1, what=" re-recorded at another offset")


# ------------------------------------------------------------------------------------------------------------------------ the step
def chain_case(chain, idx):
    """A chain recorded in the benchmarked step (test_gpu_conv_exact._step_forward: the conv2d calls one BlockCache.run recorded, with
    their views and pointers) as a case of this module: same shapes, channel strides and offsets, same dataflow (which call reads
    which input slice / earlier result, what is written in place), exact data, ReLU in place of SiLU, 1/2 for a learned scale."""
    calls = chain["calls"]
    stor = {}  # storage pointer of an input -> key
    inputs = {}
    (B, _, H, W) = calls[0]["srcs"][0][0]
    for i, (view, sp) in enumerate(chain["ins"]):
        if sp not in stor:
            stor[sp] = f"in{len(stor)}"
            inputs[stor[sp]] = BC.X(view[1])  # the whole pixel row of the storage: cstride channels
    made = []  # (key, data_ptr, channels, cstride)

    def spec(view, ptrs):
        (shape, cs, off), (dp, sp) = view, ptrs
        if sp in stor:
            return (stor[sp], off, off + shape[1])
        for key, p0, ch, cs0 in reversed(made):
            d = (dp - p0) // 2
            if cs0 == cs and 0 <= d and d + shape[1] <= ch:
                return key if (d == 0 and shape[1] == ch) else (key, d, d + shape[1])
        raise AssertionError(f"chain {chain['tag']}: a tensor of the chain is neither an input nor an earlier result")
    nodes, outs, layout = [], [], {}
    for j, cl in enumerate(calls):
        assert cl["k"] == 1 and cl["s"] == 1 and cl["ngroup"] == 1 and not any(cl["up"]) and cl["addz"] is None, cl
        key = f"s{j}"
        srcs = [spec(v, p) for v, p in zip(cl["srcs"], cl["ptrs"]["srcs"])]
        res = spec(cl["res"], cl["ptrs"]["res"]) if cl["res"] is not None else None
        (oshape, ocs, ooff), (odp, osp) = cl["out"], cl["ptrs"]["out"]
        into = (stor[osp], ooff) if osp in stor else None
        nodes.append(BC.conv(key, srcs, cl["cout"], act=BC.RELU if cl["act"] == R.ACT_SILU else cl["act"], res=res, into=into,
                             out_scale=0.5 if cl["out_scale"] != 1.0 else 1.0))
        made.append((key, odp, cl["cout"], ocs))
        if odp in chain["outs"]:
            outs.append(key)
            if ocs != cl["cout"]:
                layout[key] = (ocs, ooff)
    assert len(outs) == len(chain["outs"]), "an output of the chain is not the result of one of its convs"
    c = BC.case(f"step_{idx}_{chain['tag']}", B, H, W, inputs, nodes, outs, True,
                check_inputs=[(n["into"][0], n["into"][1], n["out"]) for n in nodes if n["into"] is not None])
    c["out_layout"] = layout
    return c


def replay_step_chain(chain, idx):
    c = chain_case(chain, idx)
    r = Run(c, tag=chain["tag"])
    ins, ov = r.dev_inputs(), r.out_views()
    got = r.launch(ins, ov)
    st = r.check_program()
    r.check(got, ins, ov)
    return [s.tile_nti for s in st]
