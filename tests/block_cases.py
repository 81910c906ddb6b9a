"""Case tables of the block-program fp64 tests (csrc/block.hip), shared by test_block_ref_cpu.py (no GPU: proves the data recipe
and the tile span) and test_gpu_block_exact.py (runs them on the kernels).

A case is a small program in ordinary operator terms: named input tensors and a list of stages that name their sources by key,
`(key, lo, hi)` being a channel slice.  `make` turns a case into data (exact dyadic or general) and the fp64_ref.gnode list.
Exact recipe: integer inputs in [-2, 2]; a stage that reads only inputs takes sparse weights in multiples of 1/4, a stage that
reads an intermediate takes two +-1 taps per output (the resolution of the values stays 1/4 through any depth, the magnitude
grows by sqrt(2) per stage on average), biases / residuals in multiples of 1/4: every partial sum is exact in fp32 in any order and
every intermediate exact in f16 -- test_block_ref_cpu.py asserts the latter for every case here."""
import zlib

import torch

import fp64_ref as R

NONE, SILU, RELU = R.ACT_NONE, R.ACT_SILU, R.ACT_RELU


# ---------------------------------------------------------------------------------------------- host-side mirrors of ey_block_compile
def conv_nt(cout):
    """conv_nt of csrc/conv_dispatch.inc.h: 16-channel row blocks per packed block tile."""
    for lim, nt in ((16, 1), (32, 2), (64, 4), (80, 5), (128, 8)):
        if cout <= lim:
            return nt
    return 8 if cout % 128 == 0 else 5 if cout % 80 == 0 else 4 if cout % 64 == 0 else 8


def tile_nti(cout):
    """tile_conv<NTI> a 1x1 stage takes in block_tile_kernel: the widest of 5, 4, 2, 1 dividing NT that leaves >= 4 items."""
    nt = conv_nt(cout)
    nblk = -(-cout // (16 * nt))
    for c in (5, 4, 2, 1):
        if nt % c == 0 and (c != 5 or nt == 5) and (nblk * (nt // c) >= 4 or c == 1):
            return c


def blk_tile(M, cout, ngroup=1):
    """(MT, NTI) of blk_conv the cost loop of ey_block_compile picks for M output pixels per image."""
    nt = conv_nt(cout)
    nblk = -(-cout // (16 * nt))
    best = None
    for mt in (1, 2, 4):
        for nti in range(1, 6):
            if nt % nti or nti == 3 or mt * nti > 8 or (nti == 5 and mt > 1):
                continue
            items = ngroup * -(-M // (16 * mt)) * nblk * (nt // nti)
            cost = -(-items // 16) * (mt + nti) * 16 + mt * nti
            if best is None or cost < best[0]:
                best = (cost, mt, nti)
    return best[1:]


TILE_NTIS = {1, 2, 4, 5}
BLK_TILES = {(1, 1), (1, 2), (1, 4), (1, 5), (2, 1), (2, 2), (2, 4), (4, 1), (4, 2)}  # the blk_conv<MT,NTI> block_kernel instantiates


# ---------------------------------------------------------------------------------------------- spec constructors
def X(C, pad=0, hw=None, kind="x"):
    """input tensor: C channels; pad > 0: a channel slice of a NaN-filled wider buffer; hw: a map of another size (addz);
    kind: x (integers), res (multiples of 1/4), neg (all negative), special (general + inf / f16 max), randn, probe"""
    return dict(C=C, pad=pad, hw=hw, kind=kind)


def conv(out, srcs, cout, k=1, s=1, act=NONE, bias=True, res=None, addz=None, out_scale=1.0, into=None, ngroup=1, w_sets=1, wkind=None):
    return dict(op="conv", out=out, srcs=list(srcs), cout=cout, k=k, s=s, act=act, bias=bias, res=res, addz=addz, out_scale=out_scale, into=into,
                ngroup=ngroup, w_sets=w_sets, wkind=wkind)


def dw(out, src, k, act=NONE, bias=True):
    return dict(op="dw", out=out, srcs=[src], k=k, act=act, bias=bias)


def ds(out, src, cout, k, act=NONE, res=None):
    """DSConv as nn._ops.dsconv records it: depthwise (bias, no activation) -> f16 -> pointwise"""
    return dict(op="ds", out=out, srcs=[src], cout=cout, k=k, act=act, res=res)


def dwt(out, src):
    return dict(op="dwt", out=out, srcs=[src])


def pool(out, src):
    return dict(op="pool", out=out, srcs=[src])


def case(name, B, H, W, inputs, nodes, outs, tiled, out_slice=(), cap=None, probe=False, bounded=True, want=(), exact=True, check_inputs=()):
    """out_slice: outputs written into a channel slice of a sentinel-filled wider buffer.  want: the tile_nti values (tiled) or
    (MT, NTI) tiles (per image) the case is there to exercise (asserted against the mirrors, then against the compiled program).
    check_inputs: (input key, lo, stage key) -- channels of an input that a stage overwrote in place, checked like an output."""
    return dict(name=name, B=B, H=H, W=W, inputs=inputs, nodes=nodes, outs=list(outs), tiled=tiled, out_slice=set(out_slice),
                cap=cap if cap is not None else (100.0 if len(nodes) == 1 else 16.0), probe=probe, bounded=bounded and not probe, want=set(want),
                exact=exact, check_inputs=list(check_inputs))


def _key(spec):
    return spec if isinstance(spec, str) else spec[0]


def shapes(c):
    """{key: (C, h, w)} of every tensor of the case"""
    sh = {k: (v["C"],) + tuple(v["hw"] or (c["H"], c["W"])) for k, v in c["inputs"].items()}

    def chans(spec):
        return sh[spec][0] if isinstance(spec, str) else spec[2] - spec[1]
    for nd in c["nodes"]:
        _, h, w = sh[_key(nd["srcs"][0])]
        cin = sum(chans(s) for s in nd["srcs"])
        if nd["op"] == "conv":
            k, s = nd["k"], nd["s"]
            sh[nd["out"]] = (nd["cout"] * nd["ngroup"], (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1)
        elif nd["op"] == "ds":
            sh[nd["out"]] = (nd["cout"], h, w)
        elif nd["op"] == "dw":
            sh[nd["out"]] = (cin, h, w)
        elif nd["op"] == "dwt":
            sh[nd["out"]] = (4 * cin, h // 2, w // 2)
        else:
            sh[nd["out"]] = (3 * cin, h, w)
    return sh


def cin_of(c, nd):
    sh = shapes(c)
    return sum(sh[s][0] if isinstance(s, str) else s[2] - s[1] for s in nd["srcs"])


def conv_stages(c):
    """[(stage spec, Cout, output pixels, ngroup)] of the conv stages in recording order (a ds stage records dw, then a 1x1 conv)"""
    sh = shapes(c)
    return [(nd, nd["cout"], sh[nd["out"]][1] * sh[nd["out"]][2], nd.get("ngroup", 1)) for nd in c["nodes"] if nd["op"] in ("conv", "ds")]


def expected_tiles(c):
    return [tile_nti(co) if c["tiled"] else blk_tile(M, co, ng) for _, co, M, ng in conv_stages(c)]


def lds_resident(c, key):
    """tiled programs keep a tensor in LDS iff only the chain touches it: a stage result that is neither an output nor written in place"""
    return key not in c["inputs"] and key not in c["outs"] and not any(nd["out"] == key and nd.get("into") for nd in c["nodes"])


# ---------------------------------------------------------------------------------------------- data
def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def probe_pixels(M):
    """first pixel, last of the first full 32-pixel tile, first of the tail tile, last pixel, one in the middle (cycled over the batch)"""
    tail0 = (M - 1) // 32 * 32
    return [0, min(31, M - 1), tail0, M - 1, M // 2]


def _input(v, B, h, w, g, general, variant):
    C, kind = v["C"], v["kind"]
    shp = (B, C, h, w)
    if kind == "probe":
        x = torch.zeros(shp, dtype=torch.float64)
        px = probe_pixels(h * w)
        for b in range(B):
            m = px[(b + variant) % len(px)]
            x[b, :, m // w, m % w] = torch.randint(1, 3, (C,), generator=g).double() * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
        return x
    if kind == "special":
        x = (torch.randn(shp, generator=g) * 100).half().double()
        r = torch.rand(shp, generator=g)
        x[r < 0.02] = float("inf")
        x[(r >= 0.02) & (r < 0.06)] = float("-inf")
        x[(r >= 0.06) & (r < 0.08)] = 65504.0
        x[(r >= 0.08) & (r < 0.10)] = -65504.0
        return x
    if general or kind == "randn":
        return torch.randn(shp, generator=g).half().double()
    if kind == "neg":
        return torch.randint(-9, 0, shp, generator=g).double()
    x = R.ex_input(shp, g)
    return x / 4 if kind == "res" else x


def _int_weight(shape, g, nz=2):
    """nz taps of +-1 per output row (at random columns of the flattened K axis)"""
    co = shape[0]
    K = shape[1] * shape[2] * shape[3]
    w = torch.zeros((co, K), dtype=torch.float64)
    cols = torch.randint(0, K, (co, nz), generator=g)
    sign = (torch.randint(0, 2, (co, nz), generator=g) * 2 - 1).double()
    w.scatter_(1, cols, sign)  # (a repeated column keeps one tap)
    return w.view(shape)


def _perm_weight(co, ci, g):
    """one tap per output row, w[o, perm(o)] in {1, 2, -1}: a permuted, asymmetric copy of the input channels"""
    perm = torch.randperm(ci, generator=g)
    w = torch.zeros((co, ci, 1, 1), dtype=torch.float64)
    vals = torch.tensor([1.0, 2.0, -1.0])
    for o in range(co):
        w[o, perm[o % ci], 0, 0] = vals[int(torch.randint(0, 3, (1,), generator=g))]
    return w


def _weights(c, nd, cin, first, g, general):
    k, co = nd["k"], nd.get("cout")
    if nd["op"] == "dw":
        if general:
            return (torch.randn((cin, 1, k, k), generator=g) / k).half().double(), (torch.randn(cin, generator=g).float() * 0.2 if nd["bias"] else None)
        w = R.ex_weight((cin, 1, k, k), g) if first else torch.randint(-1, 2, (cin, 1, k, k), generator=g).double() * (torch.rand((cin, 1, k, k), generator=g) < 0.25)
        return w, (R.ex_bias(cin, g) if nd["bias"] else None)
    K = cin * k * k
    if general:
        return (torch.randn((co, cin, k, k), generator=g) * (2.0 / K) ** 0.5).half().double(), (torch.randn(co, generator=g).float() * 0.5 if nd["bias"] else None)
    wkind = nd["wkind"] or ("perm" if c["probe"] else "dense" if first else "int")
    if wkind == "perm":
        w = _perm_weight(co, cin, g)
    elif wkind == "dense":
        w = R.ex_sparse_weight((co, cin, k, k), g, R.safe_density(K, 25.0 if nd["addz"] is not None else c["cap"]))
    else:
        w = _int_weight((co, cin, k, k), g)
    b = None
    if nd["bias"]:
        b = torch.zeros(co) if c["probe"] else R.ex_bias(co, g)
    return w, b


def haar_taps():
    """taps of the Haar bank as dwt_kernel / blk_dwt hold them, rounded to f16: +-1/2 (LL, LH, HL, HH)"""
    from edge_yolo_amd.nn.modules import block
    return block._PywtDWT2D("haar").taps32.to(torch.float16).double()


def make(c, general=False, variant=0):
    """(inputs {key: fp64 CPU tensor}, weights {stage key: dict}, fp64_ref.gnode list).  general: randn data, SiLU in place of ReLU.
    variant: another draw of the INPUTS (same weights), for replays with other data."""
    sh = shapes(c)
    inputs = {}
    for key, v in c["inputs"].items():
        _, h, w = sh[key]
        inputs[key] = _input(v, c["B"], h, w, gen(c["name"], key, general, variant), general, variant)
    wts, nodes, dirty = {}, [], set()
    for nd in c["nodes"]:
        g = gen(c["name"], nd["out"], general)
        first = all(_key(s) in c["inputs"] and _key(s) not in dirty for s in nd["srcs"])  # (an input written in place holds a stage result)
        if nd.get("into"):
            dirty.add(nd["into"][0])
        cin = cin_of(c, nd)
        act = SILU if (general and nd.get("act") == RELU) else nd.get("act", NONE)
        if nd["op"] == "conv":
            ng = nd["ngroup"]
            assert cin % ng == 0
            sets = [_weights(c, nd, cin // ng, first, g, general) for _ in range(nd["w_sets"])]
            wts[nd["out"]] = dict(sets=sets, act=act)
            if ng == 1:
                w, b = sets[0]
            else:
                w, b = [s_[0] for s_ in sets], ([s_[1] for s_ in sets] if nd["bias"] else None)
            nodes.append(R.gnode(nd["out"], nd["srcs"], w, b, nd["k"], nd["s"], None, act, addz=nd["addz"], out_scale=nd["out_scale"], res=nd["res"],
                                 into=nd["into"], ngroup=ng))
        elif nd["op"] == "dw":
            w, b = _weights(c, nd, cin, first, g, general)
            wts[nd["out"]] = dict(w=w, b=b, act=act)
            nodes.append(R.gnode(nd["out"], nd["srcs"], w, b, nd["k"], 1, None, act, dw=True, K=nd["k"] ** 2 + 1))
        elif nd["op"] == "ds":
            wd, bd = _weights(c, dict(nd, op="dw", bias=True), cin, first, g, general)
            wp, bp = _weights(c, dict(nd, op="conv", k=1, bias=True, wkind="int", addz=None), cin, False, g, general)
            wts[nd["out"]] = dict(wd=wd, bd=bd, wp=wp, bp=bp, act=act)
            nodes.append(R.gnode(nd["out"] + ".dw", nd["srcs"], wd, bd, nd["k"], 1, None, NONE, dw=True, K=nd["k"] ** 2 + 1))
            nodes.append(R.gnode(nd["out"], [nd["out"] + ".dw"], wp, bp, 1, 1, 0, act, res=nd["res"]))
        elif nd["op"] == "dwt":
            nodes.append(R.gnode(nd["out"], nd["srcs"], op="dwt", taps=haar_taps()))
        else:
            nodes.append(R.gnode(nd["out"], nd["srcs"], op="pool"))
    return inputs, wts, nodes


# ---------------------------------------------------------------------------------------------- block_tile_kernel (pointwise chains)
def _single(name, B, H, W, cin, cout, want, pad=0, out_slice=False, res=False, addz=None, **kw):
    ins = {f"x{i}": X(ci, pad=pad if i == 0 else 0) for i, ci in enumerate(cin)}
    if res:
        ins["r"] = X(cout, kind="res", pad=pad)
    if addz:
        ins["z"] = X(cout, hw=addz)
    nd = conv("y", [f"x{i}" for i in range(len(cin))], cout, res="r" if res else None, addz="z" if addz else None, **kw)
    return case(name, B, H, W, ins, [nd], ["y"], True, out_slice=["y"] if out_slice else [], want=[want])


def _c2psa_tail(name, B, H, W, c, want):
    """the tail of C2PSA_LinearAttention: x1 = b + proj(y); x2 = x1 + ffn1(ffn0(x1)) written over b inside t; cv2([a | x2])"""
    nodes = [conv("x1", ["y"], c, res=("t", c, 2 * c)), conv("f", ["x1"], 2 * c, act=RELU), conv("x2", ["f"], c, res="x1", into=("t", c)),
             conv("o", ["t"], 2 * c, act=RELU)]
    return case(name, B, H, W, dict(y=X(c, pad=16), t=X(2 * c)), nodes, ["o"], True, out_slice=["o"], want=want, check_inputs=[("t", c, "x2")])


def _eight(n):
    nodes = [conv("h0", ["x"], 8, act=RELU)]
    for i in range(1, n):
        nodes.append(conv(f"h{i}", [f"h{i - 1}"], 8, res="x" if i % 3 == 1 else (f"h{i - 2}" if i % 3 == 2 else None)))
    return nodes


TILE_CASES = [
    # ---- every tile_conv<NTI> as a single stage; Cout / Cin tails; k-step counts off the load batch (U = 8 below NTI 4, else 4)
    _single("s_nti1_cout24", 2, 3, 5, [8], 24, 1, pad=16, out_slice=True, act=RELU),
    _single("s_nti1_cout40", 5, 1, 1, [24], 40, 1),
    _single("s_nti1_cout72", 2, 13, 17, [72], 72, 1),                                   # 3 k-steps
    _single("s_nti2_cout104", 1, 13, 17, [40], 104, 2, pad=16, res=True),               # Cout tail inside the block tile, res from global
    _single("s_nti2_cout128_9ks", 2, 20, 20, [288], 128, 2),                             # 9 k-steps: one past a full batch of 8
    _single("s_nti2_cout192_2src", 5, 3, 5, [40, 24], 192, 2, pad=16),                   # global + global, both with channel tails
    _single("s_nti4_cout136", 2, 13, 17, [72], 136, 4, out_slice=True),                  # second block tile holds 8 of 128 channels
    _single("s_nti4_cout256_5ks", 1, 20, 20, [160], 256, 4),                             # 5 k-steps: one past a full batch of 4
    _single("s_nti4_cout512", 1, 3, 5, [32], 512, 4),
    _single("s_nti5_cout320", 2, 13, 17, [72], 320, 5, res=True, out_scale=0.5),
    # ---- addz: a map of another size (half: taps 1/4, 3/4; quarter: 1/8 .. 7/8; clamped edge rows / columns), out_scale != 1 (the
    # general branch of blk_epilogue) and == 1
    _single("s_addz_half_scale", 2, 20, 20, [32], 64, 1, addz=(10, 10), out_scale=0.5, act=RELU),
    _single("s_addz_quarter_relu", 2, 8, 12, [40], 40, 1, addz=(2, 3), act=RELU, pad=16),
    # ---- chains
    case("c_lds_tails", 2, 13, 17, dict(x=X(24, pad=16), r=X(24, kind="res")),
         [conv("h1", ["x"], 40, act=RELU), conv("h2", ["h1"], 72), conv("h3", ["h2", "h1"], 136, act=RELU),          # LDS Cin 40; LDS + LDS
          conv("y", [("h3", 8, 80)], 24, res="r")], ["y"], True, out_slice=["y"], want=[1, 4]),                      # slice of an LDS tensor, Cin 72
    case("c_mixed_sources", 1, 20, 20, dict(x=X(72)),
         [conv("h1", ["x"], 128, act=RELU), conv("h2", ["x", "h1"], 128, res="h1"),                                   # global + LDS, res in LDS
          conv("y5", ["h2", "x"], 320), conv("y4", ["h2"], 256, act=RELU)], ["y5", "y4"], True, want=[2, 5, 4]),      # LDS + global; two outputs
    _c2psa_tail("c_tail_inplace_c40", 5, 3, 5, 40, [1]),
    _c2psa_tail("c_tail_inplace_c128", 2, 13, 17, 128, [2, 4]),
    case("c_addz_in_chain", 2, 8, 12, dict(x=X(32), z=X(32, hw=(4, 6))),
         [conv("h", ["x"], 32, act=RELU), conv("y", ["h"], 32, addz="z", out_scale=0.5, res="x")], ["y"], True, want=[1]),
    case("c_eight_stages", 2, 3, 5, dict(x=X(8, kind="res")), _eight(8), ["h7"], True, want=[1]),
    # ---- single-tap probes: a permuted copy; a row mix-up inside a tile is named by position
    case("p_single", 5, 13, 17, dict(x=X(64, kind="probe")), [conv("y", ["x"], 64)], ["y"], True, probe=True, want=[1]),
    case("p_chain", 5, 20, 20, dict(x=X(128, kind="probe")), [conv("h", ["x"], 128), conv("y", ["h"], 256)], ["y"], True, probe=True, want=[2, 4]),
]
# refused as a pointwise chain (BlockCache.run returns None; the caller runs the same stages one launch per conv)
TILE_REFUSED = [
    case("r_nine_stages", 2, 3, 5, dict(x=X(8, kind="res")), _eight(9), ["h8"], True),
    case("r_lds_66k", 1, 3, 5, dict(x=X(8)), [conv("h1", ["x"], 512), conv("h2", ["h1"], 512), conv("y", ["h2"], 8)], ["y"], True),  # 2 x 32 x 520 halves
]


# ---------------------------------------------------------------------------------------------- block_kernel (one workgroup per image)
def _bconv(name, B, H, W, cin, cout, want, k=1, s=1, pad=0, out_slice=False, res=False, addz=None, ngroup=1, w_sets=1, **kw):
    ins = {f"x{i}": X(ci * ngroup, pad=pad if i == 0 else 0) for i, ci in enumerate(cin)}
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    if res:
        ins["r"] = X(cout * ngroup, kind="res", hw=(Ho, Wo))
    if addz:
        ins["z"] = X(cout * ngroup, hw=addz)
    nd = conv("y", [f"x{i}" for i in range(len(cin))], cout, k=k, s=s, res="r" if res else None, addz="z" if addz else None, ngroup=ngroup,
              w_sets=w_sets, **kw)
    return case(name, B, H, W, ins, [nd], ["y"], False, out_slice=["y"] if out_slice else [], want=[want])


BLOCK_CONV_CASES = [
    # k-steps per item: U = 4 (MT + NTI <= 3), 3 (<= 5), 2 (above)
    _bconv("b_1x1_k1", 2, 1, 1, [40], 40, (1, 1), pad=16, act=RELU),                               # 2 k-steps of U 4
    _bconv("b_1x1_k3_s2", 2, 1, 1, [24], 24, (1, 1), k=3, s=2),                                    # 9 k-steps
    _bconv("b_1x2_k3", 2, 13, 17, [8], 24, (1, 2), k=3, out_slice=True, res=True),                 # 9 k-steps of U 4, Cin 8
    _bconv("b_1x4_g4_sets2", 2, 3, 5, [40], 136, (1, 4), ngroup=4, w_sets=2, res=True),            # groups, two weight sets, res per group
    _bconv("b_1x5_k3_s2", 2, 25, 33, [24], 72, (1, 5), k=3, s=2, pad=16),                          # 9 k-steps of U 2
    _bconv("b_1x5_2src", 1, 7, 5, [40, 72], 320, (1, 5), pad=16),                                  # two sources, two channel strides; 2 + 3 k-steps
    _bconv("b_2x1_k3", 2, 20, 20, [72], 16, (2, 1), k=3, act=RELU),                                # 27 k-steps of U 4
    _bconv("b_2x1_2src", 3, 7, 9, [24, 8], 72, (2, 1), out_slice=True),                            # 2 k-steps
    _bconv("b_2x2_k3_s2", 2, 13, 17, [40], 192, (2, 2), k=3, s=2, res=True),                       # 18 k-steps of U 3? (MT + NTI = 4)
    _bconv("b_2x2_addz", 2, 20, 20, [32], 24, (2, 2), addz=(10, 10), out_scale=0.5),
    _bconv("b_2x4_k1", 2, 13, 17, [72], 104, (2, 4), pad=16, out_slice=True),                      # 3 k-steps of U 2, Cout tail
    _bconv("b_4x1_g4_sets1", 2, 13, 17, [24], 16, (4, 1), k=3, ngroup=4, w_sets=1),                # groups sharing one weight set
    _bconv("b_4x1_k1", 5, 10, 10, [136], 80, (4, 1)),                                              # 5 k-steps of U 3
    _bconv("b_4x2_g4_addz", 2, 20, 20, [32], 24, (4, 2), ngroup=4, w_sets=2, addz=(10, 10), act=RELU),  # groups with addz
    _bconv("b_4x2_g4_k3_res", 1, 13, 17, [8], 32, (4, 2), k=3, ngroup=4, w_sets=2, res=True, out_scale=0.5),
]

BLOCK_OP_CASES = [
    # ---- depthwise k 3 / 5 / 7, bias / none, act none / ReLU (bounded run: SiLU), odd maps smaller than the kernel
    case("d_dw3", 2, 13, 17, dict(x=X(80, pad=16)), [dw("y", "x", 3, act=RELU)], ["y"], False, out_slice=["y"]),
    case("d_dw5_nobias", 3, 7, 5, dict(x=X(24)), [dw("y", "x", 5, bias=False)], ["y"], False),
    case("d_dw7_small_map", 2, 3, 3, dict(x=X(8)), [dw("y", "x", 7, act=RELU)], ["y"], False),
    case("d_dw7", 1, 20, 20, dict(x=X(24)), [dw("y", "x", 7)], ["y"], False),
    case("d_dsconv5_res", 2, 13, 17, dict(x=X(40)), [ds("y", "x", 40, 5, act=RELU, res="x")], ["y"], False, want=[blk_tile(221, 40)]),
    case("d_dsconv3", 2, 7, 5, dict(x=X(24, pad=16)), [ds("y", "x", 72, 3)], ["y"], False, out_slice=["y"], want=[blk_tile(35, 72)]),
    # ---- Haar DWT (NaN-slice input, sentinel output; odd maps drop the last row / column)
    case("w_dwt_even", 2, 10, 14, dict(x=X(16, pad=16)), [dwt("y", "x")], ["y"], False, out_slice=["y"]),
    case("w_dwt_odd", 3, 9, 13, dict(x=X(8, pad=16)), [dwt("y", "x")], ["y"], False, out_slice=["y"]),
    case("w_dwt_min", 2, 2, 2, dict(x=X(40)), [dwt("y", "x")], ["y"], False),
    # ---- SPPF pool chain: exact for any data
    case("m_pool_general", 2, 13, 17, dict(x=X(24, pad=16, kind="randn")), [pool("y", "x")], ["y"], False, out_slice=["y"], bounded=False),
    case("m_pool_negative", 2, 7, 5, dict(x=X(8, kind="neg")), [pool("y", "x")], ["y"], False, bounded=False),
    case("m_pool_inf", 2, 9, 6, dict(x=X(16, kind="special")), [pool("y", "x")], ["y"], False, bounded=False),
    case("m_pool_1x1", 3, 1, 1, dict(x=X(8, kind="randn")), [pool("y", "x")], ["y"], False, bounded=False),
    case("m_pool_chunks", 1, 20, 20, dict(x=X(136, kind="randn")), [pool("y", "x")], ["y"], False, bounded=False),  # 17 octets, 8 per LDS chunk: 8 + 8 + 1
    # ---- a mixed program, end to end
    case("x_mixed", 2, 20, 20, dict(x=X(24, pad=16)),
         [conv("a", ["x"], 40, k=3, s=2, act=RELU), dw("d", "a", 3), conv("c", ["d"], 40, res="a", act=RELU), dwt("w", "c"), pool("p", "w"),
          conv("y", ["p"], 72)], ["y"], False, out_slice=["y"], cap=8.0),
]
BLOCK_CASES = BLOCK_CONV_CASES + BLOCK_OP_CASES
ALL_CASES = TILE_CASES + BLOCK_CASES
BY_NAME = {c["name"]: c for c in ALL_CASES + TILE_REFUSED}
assert len(BY_NAME) == len(ALL_CASES) + len(TILE_REFUSED)
