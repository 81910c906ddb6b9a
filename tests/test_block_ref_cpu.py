"""No GPU: the graph reference of tests/fp64_ref.py (graph_ref) and the case tables of tests/block_cases.py.

* on a straight chain graph_ref returns exactly chain_ref's y and bound;
* on the C2PSA tail (in-place write over a slice of an input, two-source read-back) with f16_points=False it equals a plain float64
  composition written with torch.nn.functional.conv2d;
* for EVERY exact case of the GPU matrix the fp64 graph is evaluated here and every intermediate and output is exactly
  representable in f16 -- the precondition of fp64_ref.assert_exact: a GPU failure is then the kernel's, not the data recipe's;
* the host-side mirrors of ey_block_compile say that the tables span the four tile_conv<NTI> and the nine blk_conv<MT,NTI>."""
import pytest
import torch
import torch.nn.functional as F

import block_cases as BC
import fp64_ref as R


def test_graph_equals_chain_ref_on_a_line():
    g = BC.gen("line")
    x = torch.randn((2, 24, 7, 9), generator=g).half().double()
    r = torch.randn((2, 16, 7, 9), generator=g).half().double()
    z = torch.randn((2, 40, 3, 4), generator=g).half().double()
    w1 = (torch.randn((40, 24, 3, 3), generator=g) * 0.1).half().double()
    wd = (torch.randn((40, 1, 5, 5), generator=g) * 0.2).half().double()
    w3 = (torch.randn((16, 40, 1, 1), generator=g) * 0.2).half().double()
    b1, bd, b3 = torch.randn(40, generator=g), torch.randn(40, generator=g), torch.randn(16, generator=g)
    stages = [R.stage(w1, b1, 3, 1, 1, R.ACT_SILU, addz=z, out_scale=0.5), R.stage(wd, bd, 5, 1, 2, R.ACT_NONE, dw=True, K=26),
              R.stage(w3, b3, 1, 1, 0, R.ACT_RELU, res=r)]
    per_stage = []
    y, bnd = R.chain_ref([x], stages, on_stage=lambda i, yy, bb: per_stage.append((yy, bb)))
    nodes = [R.gnode("a", ["x"], w1, b1, 3, 1, 1, R.ACT_SILU, addz="z", out_scale=0.5), R.gnode("b", ["a"], wd, bd, 5, 1, 2, R.ACT_NONE, dw=True, K=26),
             R.gnode("c", ["b"], w3, b3, 1, 1, 0, R.ACT_RELU, res="r")]
    ref = R.graph_ref(dict(x=x, r=r, z=z), nodes)
    assert torch.equal(ref["c"][0], y) and torch.equal(ref["c"][1], bnd)
    for key, (yy, bb) in zip("abc", per_stage):
        assert torch.equal(ref[key][0], yy) and torch.equal(ref[key][1], bb), key
    y0, b0 = R.chain_ref([x], stages, f16_points=False)
    ref0 = R.graph_ref(dict(x=x, r=r, z=z), nodes, f16_points=False)
    assert torch.equal(ref0["c"][0], y0) and torch.equal(ref0["c"][1], b0)


def test_graph_c2psa_tail_equals_plain_fp64_composition():
    c = BC.BY_NAME["c_tail_inplace_c40"]
    inputs, wts, nodes = BC.make(c, general=True)
    ref = R.graph_ref(inputs, nodes, f16_points=False)
    ch = 40
    y, t = inputs["y"], inputs["t"]

    def cv(x, key):
        w, b = wts[key]["sets"][0]
        v = F.conv2d(x, w, b.double())
        return v * torch.sigmoid(v) if wts[key]["act"] == R.ACT_SILU else v
    a, b = t[:, :ch], t[:, ch:]
    x1 = b + cv(y, "x1")
    x2 = x1 + cv(cv(x1, "f"), "x2")
    o = cv(torch.cat([a, x2], 1), "o")
    assert wts["f"]["act"] == R.ACT_SILU and wts["o"]["act"] == R.ACT_SILU
    for key, want in (("x1", x1), ("x2", x2), ("o", o)):
        got = ref[key][0]
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), key
    # with the f16 points the bound of the last stage carries the error of x2 read back from the input it was written over
    refh = R.graph_ref(inputs, nodes)
    assert bool((refh["o"][1] > R.bound(*R.conv_ref([torch.cat([a, x2], 1)], wts["o"]["sets"][0][0], wts["o"]["sets"][0][1], act=R.ACT_SILU), 81)).all())


@pytest.mark.parametrize("name", [c["name"] for c in BC.ALL_CASES + BC.TILE_REFUSED if c["exact"]])
def test_exact_cases_are_exact_in_f16(name):
    """every stage result of the fp64 graph (outputs and chain-internal tensors) is an f16 value, for both input draws the replay
    tests use: what the kernels keep as f16 loses nothing, and partial sums of quarter-integers below 2^11 are exact in fp32"""
    c = BC.BY_NAME[name]
    for variant in (0, 1, 2):
        inputs, _, nodes = BC.make(c, variant=variant)
        seen = []

        def on_node(nd, y, bnd):
            assert torch.equal(y.to(torch.float16).double(), y), f"{name}: stage {nd['out']} is not exact in f16 (max |y| {float(y[torch.isfinite(y)].abs().max())})"
            if nd["op"] != "pool":
                assert float((y * 64).frac().abs().max()) == 0 and float(y.abs().max()) < 2048, f"{name}: stage {nd['out']} leaves the dyadic recipe"
            seen.append(nd["out"])
        R.graph_ref(inputs, nodes, on_node=on_node)
        assert len(seen) == len(nodes)


def test_probe_outputs_are_permuted_copies():
    for name in ("p_single", "p_chain"):
        c = BC.BY_NAME[name]
        inputs, _, nodes = BC.make(c)
        y = R.graph_ref(inputs, nodes)[c["outs"][0]][0]
        M = c["H"] * c["W"]
        for b in range(c["B"]):
            m = BC.probe_pixels(M)[b % 5]
            nz = y[b].abs().sum(0).flatten().nonzero().flatten().tolist()
            assert nz == [m], (name, b, nz, m)


def test_tables_span_every_instantiation():
    nti = set()
    for c in BC.TILE_CASES:
        exp = set(BC.expected_tiles(c))
        assert c["want"] <= exp, f"{c['name']}: meant for tile_nti {sorted(c['want'])}, the compile rule gives {sorted(exp)}"
        nti |= exp
    assert nti == BC.TILE_NTIS, nti
    tiles = set()
    for c in BC.BLOCK_CASES:
        exp = set(BC.expected_tiles(c))
        assert c["want"] <= exp, f"{c['name']}: meant for blk_conv {sorted(c['want'])}, the cost loop gives {sorted(exp)}"
        tiles |= exp
    assert tiles == BC.BLK_TILES, sorted(tiles)
    # the rule as the issue lists it
    assert [BC.tile_nti(co) for co in (24, 40, 72, 80, 128, 192, 256, 512, 320)] == [1, 1, 1, 1, 2, 2, 4, 4, 5]


def test_tiled_cases_place_tensors_as_meant():
    """the placements the tiled matrix is there for exist in the table (the GPU test asserts them on the compiled program)"""
    kinds = set()
    for c in BC.TILE_CASES:
        for nd in c["nodes"]:
            place = tuple("L" if BC.lds_resident(c, BC._key(s)) else "G" for s in nd["srcs"])
            kinds.add(("src",) + place)
            for s in nd["srcs"]:
                if not isinstance(s, str) and s[1] > 0 and BC.lds_resident(c, s[0]):
                    kinds.add("lds_slice")
                cin = BC.shapes(c)[s][0] if isinstance(s, str) else s[2] - s[1]
                if cin % 32:
                    kinds.add(("cin_tail", "L" if BC.lds_resident(c, BC._key(s)) else "G"))
            if nd["res"] is not None:
                kinds.add(("res", "L" if BC.lds_resident(c, BC._key(nd["res"])) else "G"))
            if nd["into"] is not None:
                kinds.add("inplace")
    for want in (("src", "G", "G"), ("src", "G", "L"), ("src", "L", "G"), ("src", "L", "L"), "lds_slice", ("cin_tail", "L"), ("cin_tail", "G"), ("res", "L"),
                 ("res", "G"), "inplace"):
        assert want in kinds, want
    for c in BC.TILE_REFUSED:
        assert len(c["nodes"]) == 9 or sum(32 * (nd["cout"] + 8) * 2 for nd in c["nodes"] if BC.lds_resident(c, nd["out"])) > 56 * 1024
    assert len(BC.BY_NAME["c_eight_stages"]["nodes"]) == 8
