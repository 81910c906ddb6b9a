"""The shared builders of nn/modules/block.py and the input gather of nn/tasks.py, without a device: stacked and repeated 1x1 weights, the
per-channel scale vector, the chain caches of _Chains, _inputs, and the forward signatures that lost an argument."""
import inspect
import types

import pytest
import torch

import synthdata as synth


@pytest.fixture(scope="module")
def B():
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd.nn.modules import block
    return block


def _convs(B, couts, cin=8):
    convs = [B.Conv(cin, c, 1) for c in couts]
    for i, m in enumerate(convs):
        m.load_state_dict({k: synth.synth_tensor(f"stack{i}.{k}", tuple(v.shape)) for k, v in m.state_dict().items()})
    return convs


@pytest.mark.parametrize("couts", [(8, 16), (8, 8, 16, 24)])
def test_stacked_is_the_cat_of_the_members_folded(B, couts):
    convs = _convs(B, couts)
    for fused in (False, True):
        if fused:
            for m in convs:
                m.fuse_bn()
            assert not any(hasattr(m, "bn") for m in convs)
        w, b = B._stacked(*convs)
        ws, bs = zip(*(m.folded() for m in convs))
        assert torch.equal(w, torch.cat(ws, 0)) and torch.equal(b, torch.cat(bs, 0))
        assert w.shape == (sum(couts), 8, 1, 1) and b.shape == (sum(couts),) and w.dtype == b.dtype == torch.float32


def test_c3_cv12_and_its_activation(B):
    m = B.C3(16, 16, 1)
    w, b = m._cv12()
    (w1, b1), (w2, b2) = m.cv1.folded(), m.cv2.folded()
    assert torch.equal(w, torch.cat((w1, w2), 0)) and torch.equal(b, torch.cat((b1, b2), 0))
    assert m._cv12_act() == B._act_code(m.cv1.act) == B._stacked_act(m.cv1, m.cv2)
    m.cv2.act = torch.nn.Identity()
    assert B._stacked_act(m.cv1, m.cv2) is None and B._stacked_act(m.cv1) == B._act_code(m.cv1.act)
    with pytest.raises(NotImplementedError):
        m._cv12_act()


def test_repeated_is_the_weight_twice_along_cin(B):
    conv, = _convs(B, (16,))
    w, b = conv.folded()
    w2, b2 = B._repeated(conv)
    assert torch.equal(w2, torch.cat((w, w), 1)) and torch.equal(b2, b) and w2.shape == (16, 16, 1, 1)


@pytest.mark.parametrize("shape", [(), (1,), (6,)])
def test_scale_vec(B, shape):
    C = 6
    mod = B.FullPAD_Tunnel()
    p = torch.nn.Parameter(torch.full(shape, 0.1) + 1e-4 * torch.arange(C if shape == (C,) else 1).reshape(shape))  # (not representable in f16)
    x = torch.zeros(2, C, 3, 3, dtype=torch.float16)
    v = B._scale_vec(mod, "gate", p, x)
    assert v.dtype == torch.float32 and v.shape == (C,) and v.is_contiguous() and not v.requires_grad
    assert torch.equal(v, p.detach().half().float().expand(C)) and not torch.equal(v, p.detach().expand(C))
    assert B._scale_vec(mod, "gate", p, x) is v
    assert B._scale_vec(mod, "gate", p, x.float()) is not v  # another dtype, another rounding
    assert torch.equal(B._scale_vec(mod, "gate", p, x.float()), p.detach().expand(C))


def test_ablock_is_packed_without_a_state_dict_key(B):
    m = B.ABlock(32, 1, mlp_ratio=1.2)
    assert isinstance(m, B._Packed) and not any("_cache" in k or "ones" in k for k in m.state_dict())
    x = torch.zeros(1, 32, 2, 2, dtype=torch.float16)
    assert torch.equal(B._scale_vec(m, "ones", torch.ones(()), x), torch.ones(32))


def test_chain_caches_drop_with_the_parameters(B):
    m = B.C2PSA_LinearAttention(64, 64)
    assert isinstance(m, B._Packed) and "_apply" not in vars(B._Chains) and "_load_from_state_dict" not in vars(B._Chains)
    c = m._chain("proj_ffn_cv2")
    assert m._chain("proj_ffn_cv2") is c and m._chain("cv1_qkv") is not c and m._cache[("chain", "proj_ffn_cv2")] is c
    m.half()
    assert ("chain", "proj_ffn_cv2") not in m._cache
    c2 = m._chain("proj_ffn_cv2")
    assert c2 is not c
    m.load_state_dict(m.state_dict())
    assert m._chain("proj_ffn_cv2") is not c2
    assert m.pw_chains == ("proj_ffn_cv2",) and not m._chains_on(torch.zeros(1, 64, 4, 4, dtype=torch.float16))  # (a CPU tensor never chains)


def test_linear_attention_folding(B):
    at = B.LinearAttention(32, 1, qkv_bias=True, proj_bias=False)
    w, b = at._proj_folded()
    assert b is None and torch.equal(w, at.proj.weight.detach().float())  # a missing bias stays None: it must not become zeros
    w, b = at._qkv_folded()
    assert torch.equal(w, at.qkv.weight.detach().float()) and torch.equal(b, at.qkv.bias.detach().float())
    w, b = B.LinearAttention(32, 1, qkv_bias=False, proj_bias=True)._proj_folded()
    assert b is not None and b.shape == (32,)


def test_inputs_gathers_from_x_and_the_saved_outputs():
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd.nn.tasks import _inputs
    x, y = object(), [object(), None, object()]
    assert _inputs(types.SimpleNamespace(f=-1), x, y) is x
    assert _inputs(types.SimpleNamespace(f=2), x, y) is y[2]
    got = _inputs(types.SimpleNamespace(f=[-1, 0, 2]), x, y)
    assert isinstance(got, list) and len(got) == 3 and got[0] is x and got[1] is y[0] and got[2] is y[2]


def test_forwards_that_lost_an_argument(B):
    assert list(inspect.signature(B.C2f.forward).parameters) == ["self", "x", "out"]
    assert list(inspect.signature(B.SPPF.forward).parameters) == ["self", "x", "out"]
    assert "tail" in inspect.signature(B.DSC3K2_Wavelet.forward).parameters
    assert "forward" not in vars(B.C2fAttn) and "forward" not in vars(B.DSC3K2)
    for name in ("_DSUnit", "_LGLAdapter", "_DSUnitWithLGL"):
        assert name not in B.__all__ and hasattr(B, name)
