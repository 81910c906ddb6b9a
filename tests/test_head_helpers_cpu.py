"""CPU-only tests of the host helpers the detection heads share (nn/modules/head.py): the tower stream map, the level builder, the cache
keys and their resets, and the structure predicate of the light class tower.  No kernel is launched here."""
import pytest
import torch
import torch.nn as nn

import edge_yolo_amd  # noqa: F401
from edge_yolo_amd.nn import _ops
from edge_yolo_amd.nn.modules import head as H
from edge_yolo_amd.nn.modules.conv import Conv, DWConv

CPU = torch.device("cpu")


class Light(H.Detect):
    legacy = False  # parse_model assigns `legacy` on the head class (reference tasks.py:1096): pinned here, whatever model was built before


class Legacy(H.Detect):
    legacy = True


@pytest.mark.parametrize("n", [1, 3, 4])
def test_stream_map_default(n):
    """The first level on the caller's stream, every smaller level on ONE side stream."""
    h = H.Detect(nc=8, ch=(16,) * n)
    assert h._stream_map(n) == [0, 0] + [1] * (2 * n - 2)
    assert len(h._stream_map(n)) == 2 * n


def test_stream_map_takes_tower_streams_of_length_2n_only():
    h = H.Detect(nc=8, ch=(16, 32))
    h.tower_streams = (0, 1, 2, 0)
    assert h._stream_map(2) == [0, 1, 2, 0]
    assert h._stream_map(3) == [0, 0, 1, 1, 1, 1]  # another length: ignored
    h.tower_streams = (0, 1, 2)
    assert h._stream_map(2) == [0, 0, 1, 1]
    h.tower_streams = ()
    assert h._stream_map(2) == [0, 0, 1, 1]


@pytest.mark.parametrize("cls", [H.Detect, H.GF2Detect])
def test_level_builder_strides_and_offsets(cls):
    h = cls(nc=8, ch=(16, 32, 64))
    h.stride = torch.tensor([8.0, 16.0, 32.0])
    sizes = [(4, 6), (2, 3), (1, 2)]
    maps = [(torch.zeros(2, 64, hh, ww), torch.zeros(2, 8, hh, ww)) for hh, ww in sizes]
    levels = h._levels(maps)
    assert [lv.stride for lv in levels] == [8.0, 16.0, 32.0] and all(type(lv.stride) is float for lv in levels)
    assert [lv.a_off for lv in levels] == [0, 24, 30]
    assert h._stride_f == [8.0, 16.0, 32.0]
    for i, lv in enumerate(levels):
        assert isinstance(lv, tuple) and isinstance(lv, _ops.Level) and len(lv) == 5
        box, c, st, q, off = lv  # by position, as the plain 5-tuples of tests and tools
        assert box is lv.box is lv[0] is maps[i][0] and c is lv.cls is lv[1] is maps[i][1]
        assert st == lv.stride == lv[2] and q is lv.q is lv[3] and off == lv.a_off == lv[4]
        if cls is H.Detect:
            assert q is None
        else:  # (w1 [hid, 20], b1 [hid], w2 [hid], b2 [1]) fp32 of this level's quality head
            assert [tuple(t.shape) for t in q] == [(64, 20), (64,), (64,), (1,)] and q is h._qcache[("", i, CPU)]
            assert torch.equal(q[0], h.reg_conf[i][0].weight.detach().view(64, 20))
    # the keypoint level list walks the same strides and offsets
    p = H.Pose(nc=1, kpt_shape=(3, 2), ch=(16, 32, 64))
    p.stride = h.stride
    kmaps = [torch.zeros(2, 6, hh, ww) for hh, ww in sizes]
    assert [(m is kmaps[i], st, off) for i, (m, st, off) in enumerate(p.kpt_levels(kmaps))] == [(True, 8.0, 0), (True, 16.0, 24), (True, 32.0, 30)]


def test_level_builder_reads_the_branch():
    h = H.E2EDetect(nc=8, ch=(16, 32))
    h.stride = torch.tensor([8.0, 16.0])
    with torch.no_grad():
        h.one2one_reg_conf[1][0].bias.fill_(3.0)
    maps = [(torch.zeros(1, 64, 2, 2), torch.zeros(1, 8, 2, 2)), (torch.zeros(1, 64, 1, 1), torch.zeros(1, 8, 1, 1))]
    many, one = h._levels(maps), h._levels(maps, "one2one_")
    assert set(h._qcache) == {(br, i, CPU) for br in ("", "one2one_") for i in range(2)}
    assert torch.all(one[1].q[1] == 3.0) and not torch.any(many[1].q[1] == 3.0)
    assert h._quality_params(1, CPU) is many[1].q and h._quality_params(1, CPU, "one2one_") is one[1].q


def _all_tails(h, towers, branches=("",)):
    return {(br, tw, i): h._tail(tw, i, br) for br in branches for tw in towers for i in range(h.nl)}


@pytest.mark.parametrize("make,towers,branches", [
    (lambda: Light(nc=8, ch=(16, 32, 64)), ("cv2", "cv3"), ("",)),
    (lambda: Legacy(nc=8, ch=(16, 32, 64)), ("cv2", "cv3"), ("",)),
    (lambda: H.Segment(nc=8, nm=4, npr=8, ch=(16, 32, 64)), ("cv2", "cv3", "cv4"), ("",)),
    (lambda: H.E2EDetect(nc=8, ch=(16, 32, 64)), ("cv2", "cv3"), ("", "one2one_")),
], ids=["Detect", "Detect-legacy", "Segment", "E2EDetect"])
def test_tail_cache_keys_say_what_the_entry_is(make, towers, branches):
    h = make()
    tails = _all_tails(h, towers, branches)
    assert set(h._tails) == set(tails) and len(tails) == len(branches) * len(towers) * 3
    assert len({id(t) for t in tails.values()}) == len(tails)  # one packed tail per (branch, tower, level) ...
    for (br, tw, i), t in tails.items():
        assert t._ref is getattr(h, br + tw)[i][-1]  # ... of exactly that tower's closing conv
        assert h._tail(tw, i, br) is t
        w, b = t.folded()
        assert torch.equal(w, t._ref.weight.detach().float()) and torch.equal(b, t._ref.bias.detach().float())


def _dirty(h):
    h._tails[("", "cv2", 0)] = object()
    h._stride_f = [1.0]
    h.__dict__["_blk"] = {0: object()}
    if hasattr(h, "_qcache"):
        h._qcache[("", 0, CPU)] = object()


def _clean(h):
    return h._tails == {} and h._stride_f is None and h._blk == {} and getattr(h, "_qcache", {}) == {}


@pytest.mark.parametrize("cls", [H.Detect, H.GF2Detect, H.E2EDetect])
def test_caches_are_empty_after_load_state_dict_and_to(cls):
    h = cls(nc=8, ch=(16, 32))
    _dirty(h)
    h.load_state_dict(h.state_dict())
    assert _clean(h)
    _dirty(h)
    h.to(torch.float64)
    assert _clean(h)
    _dirty(h)
    h.stride = torch.tensor([8.0, 16.0])
    h.bias_init()
    assert _clean(h)


def test_world_set_text_empties_the_caches_and_moves_the_class_mask():
    h = H.WorldDetect(nc=80, embed=16, with_bn=True, ch=(16, 32))
    h.set_text(torch.randn(1, 6, 16))
    m6 = h._class_mask([0, 2], CPU)
    assert m6.tolist() == [1, 0, 1, 0, 0, 0] and h._class_mask([0, 2], CPU) is m6 and h._class_mask(None, CPU) is None
    _dirty(h)
    h._fold(0)
    h.set_text(torch.randn(1, 4, 16))
    assert _clean(h) and h.nc == 4 and h.no == 68
    assert h._class_mask([0, 2], CPU).tolist() == [1, 0, 1, 0]  # nc is part of the key: no stale 6-class mask
    from edge_yolo_amd.utils.ops import _class_mask
    assert _class_mask([0, 2], 4, CPU) is h._class_mask([0, 2], CPU)  # one implementation, one cache


def _light(mid_act=True, c3=80, nc=8):
    return nn.Sequential(nn.Sequential(DWConv(16, 16, 3), Conv(16, c3, 1)), nn.Sequential(DWConv(c3, c3, 3), Conv(c3, c3, 1, act=mid_act)), nn.Conv2d(c3, nc, 1))


def test_light_closing_predicate():
    assert H._light_closing(_light())
    assert all(H._light_closing(c) for c in Light(nc=8, ch=(16, 32)).cv3)
    assert not any(H._light_closing(c) for c in Legacy(nc=8, ch=(16, 32)).cv3)
    assert all(H._light_closing(c) for c in H.v10Detect(nc=8, ch=(16, 32)).one2one_cv3)
    legacy = nn.Sequential(Conv(16, 80, 3), Conv(80, 80, 3), nn.Conv2d(80, 8, 1))
    assert not H._light_closing(legacy)
    assert not H._light_closing(_light(mid_act=False))  # the chained kernel applies SiLU between the two 1x1 convs
    assert not H._light_closing(_light(mid_act=nn.ReLU()))
    wide = _light()
    wide[2] = nn.Conv2d(80, 8, 3, padding=1)
    assert not H._light_closing(wide)
    grouped = _light()
    grouped[2] = nn.Conv2d(80, 8, 1, groups=2)
    assert not H._light_closing(grouped)


def test_legacy_head_builds_the_legacy_tower():
    h = Legacy(nc=8, ch=(16, 32))
    assert not any(H._light_closing(c) for c in h.cv3)
    assert not h._chained(0, torch.zeros(1, 16, 2, 2, dtype=torch.float16))
    g = Light(nc=8, ch=(16, 32))
    assert g._chained(0, torch.zeros(1, 16, 2, 2, dtype=torch.float16)) and not g._chained(0, torch.zeros(1, 16, 2, 2))
    g.chain = False
    assert not g._chained(0, torch.zeros(1, 16, 2, 2, dtype=torch.float16))
