"""CPU: general PyWavelets filter banks (wave=) and use_ds=True of the wavelet blocks (reference block.py:3582-3788) -- the
filter table against PyWavelets' own coefficients, construction, state_dict keys, the YAML kwargs mapping and the weight bridge."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import synthdata as synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E():
    import edge_yolo_amd
    return edge_yolo_amd


@pytest.fixture(scope="module")
def pywt_table(golden_dir):
    return json.load(open(os.path.join(golden_dir, "pywt_filters.json")))["filters"]


def test_filter_table_equals_pywt(E, pywt_table):
    from edge_yolo_amd.nn.modules.block import wavelet_filters
    table, too_long = wavelet_filters()
    assert len(table) == 93 and set(table) == set(pywt_table)
    for name, f in pywt_table.items():
        assert table[name] == (tuple(f["dec_lo"]), tuple(f["dec_hi"])), name
    assert sorted(too_long) == sorted([f"db{i}" for i in range(33, 39)] + [f"coif{i}" for i in range(11, 18)])
    assert all(n > 64 for n in too_long.values()) and all(len(lo) <= 64 and len(lo) % 2 == 0 for lo, _ in table.values())


def test_orthogonal_identities(E):
    from edge_yolo_amd.nn.modules.block import wavelet_filters
    table, _ = wavelet_filters()
    orth = [n for n in table if n.rstrip("0123456789") in ("haar", "db", "sym", "coif")]
    assert len(orth) >= 60
    for name in orth:
        lo, hi = (np.array(v, dtype=np.float64) for v in table[name])
        assert abs(lo.sum() - math.sqrt(2)) < 1e-9, name
        assert abs((lo * lo).sum() - 1) < 1e-9, name
        k = len(lo)  # quadrature mirror: dec_hi[n] = (-1)^(n+1) dec_lo[k-1-n]
        np.testing.assert_allclose(hi, [(-1) ** (n + 1) * lo[k - 1 - n] for n in range(k)], rtol=0, atol=1e-12, err_msg=name)


@pytest.mark.parametrize("name", ["db33", "db38", "coif11", "coif17", "nosuch", "cmor1.5-1.0", "gaus1"])
def test_refused_names(E, name):
    from edge_yolo_amd.nn.modules.block import _PywtDWT2D, _WaveletEnhancer
    with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
        _PywtDWT2D(name)
    with pytest.raises(NotImplementedError):
        _WaveletEnhancer(16, wave=name)


def test_taps_follow_the_reference_rule(E, pywt_table):
    """h0 = dec_lo[::-1], h1 = dec_hi[::-1]; LL|LH|HL|HH = fp32 outer products (LH rows h0, columns h1), then cast to the dtype."""
    from edge_yolo_amd.nn.modules.block import _PywtDWT2D
    for name in ("haar", "db2", "sym4", "bior2.2", "dmey"):
        d = _PywtDWT2D(name, mode="zero")
        assert d.mode == "zero" and d.k == len(pywt_table[name]["dec_lo"]) and d.pad == d.k // 2 - 1
        h0 = torch.tensor(pywt_table[name]["dec_lo"][::-1], dtype=torch.float32)
        h1 = torch.tensor(pywt_table[name]["dec_hi"][::-1], dtype=torch.float32)
        for q, (a, b) in enumerate(((h0, h0), (h0, h1), (h1, h0), (h1, h1))):
            assert torch.equal(d.taps32[q], a[:, None] * b[None, :]), (name, q)
    assert _PywtDWT2D("haar").haar and _PywtDWT2D("db1").haar and not _PywtDWT2D("db2").haar
    assert float(_PywtDWT2D("haar").taps32[0, 0, 0]) == 0.49999997019767761


def test_reflect_pad_rule(E):
    from edge_yolo_amd.nn.modules.block import _PywtDWT2D
    d = _PywtDWT2D("dmey")  # 62 taps: pad 30
    d.check_size(31, 31)
    for hw in ((30, 40), (40, 30), (1, 8)):
        with pytest.raises(ValueError):
            d.check_size(*hw)
    _PywtDWT2D("haar").check_size(2, 2)
    with pytest.raises(ValueError, match="2x2 Haar"):
        _PywtDWT2D("haar").check_size(1, 4)


def test_use_ds_state_dict_keys_match_reference(E, golden_dir):
    from edge_yolo_amd.nn.modules.block import _WaveletEnhancer
    g = np.load(os.path.join(golden_dir, "wavelets_ops.npz"))
    m = _WaveletEnhancer(16, use_ds=True, wave="db2")
    assert sorted(m.state_dict()) == [str(k) for k in g["enh_ds_keys"]]
    assert {"f_h.dw.weight", "f_h.pw.weight", "f_h.bn.weight"} <= set(m.state_dict())


def _yaml_with_mapping(mapping):
    from edge_yolo_amd.nn.tasks import yaml_model_load
    d = dict(yaml_model_load("yolo11n-test.yaml"))
    d["backbone"] = [list(r) for r in d["backbone"]]
    d["head"] = [list(r) for r in d["head"]]
    rows = []
    for j, r in enumerate(d["backbone"] + d["head"]):
        if r[2] == "DSC3K2_Wavelet":
            r[3] = list(r[3]) + [dict(mapping)]
            rows.append(j)
    return d, rows


def test_yaml_trailing_mapping_builds_and_round_trips(E, tmp_path):
    from edge_yolo_amd.nn.modules.block import DSConv, DSC3K2_Wavelet
    d, rows = _yaml_with_mapping({"wave": "db2", "use_ds": True})
    assert rows
    y = E.YOLO(d)
    for j in rows:
        m = y.model.model[j]
        assert isinstance(m, DSC3K2_Wavelet) and m.wave.dwt.wave_name == "db2" and isinstance(m.wave.f_h, DSConv)
    y.model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in y.model.state_dict().items()}))
    f = str(tmp_path / "db2ds.pt")
    y.save(f)
    y2 = E.YOLO(f)
    for j in rows:
        m = y2.model.model[j]
        assert m.wave.dwt.wave_name == "db2" and isinstance(m.wave.f_h, DSConv)
        assert (d["backbone"] + d["head"])[j][3][-1] == {"wave": "db2", "use_ds": True}
    a, b = y.model.state_dict(), y2.model.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    bad, _ = _yaml_with_mapping({"wavelet": "db2"})
    with pytest.raises(ValueError, match="wave, use_ds and mode"):
        E.YOLO(bad)


class _Mod(torch.nn.Module):
    pass


class DSC3K2_Wavelet(torch.nn.Module):  # stand-ins named like the reference classes the export tool inspects
    pass


class DSConv(torch.nn.Module):
    pass


class Conv(torch.nn.Module):
    pass


class _RefModel(torch.nn.Module):
    """A proxy for the reference model, not the reference's own module tree: a hand-built module carrying what the reference's
    DetectionModel('yolo11n-test.yaml') with every enhancer built as _WaveletEnhancer(c, use_ds=True, wave='db2') holds, as the
    reference recorded it (tests/golden/ref_checkpoint_n_db2_ds.json): its parsed yaml (which does NOT name the wave), each enhancer's
    layer index, wave_name, mode and f_h class name, and its state_dict keys and shapes.  The reference package is not importable where
    the tests run; the exporter reads exactly these attributes (found through model.modules(), so nesting does not matter)."""

    def __init__(self, g):
        super().__init__()
        self.yaml = g["yaml"]
        n = len(g["yaml"]["backbone"]) + len(g["yaml"]["head"])
        self.model = torch.nn.ModuleList(_Mod() for _ in range(n))
        for i, w in g["waves"].items():
            m = DSC3K2_Wavelet()
            m.i = int(i)
            m.wave = _Mod()
            m.wave.dwt = _Mod()
            m.wave.dwt.wave_name, m.wave.dwt.mode = w["wave_name"], w["mode"]
            m.wave.f_h = {"DSConv": DSConv, "Conv": Conv}[w["f_h"]]()
            self.model[int(i)] = m
        self.sd = synth.synth_state_dict({k: tuple(s) for k, s in g["state_shapes"].items()})

    def state_dict(self, *a, **k):
        return dict(self.sd)


def test_export_records_wave_and_use_ds(E, tmp_path, golden_dir):
    g = json.load(open(os.path.join(golden_dir, "ref_checkpoint_n_db2_ds.json")))
    assert g["waves"] and all(w["wave_name"] == "db2" and w["f_h"] == "DSConv" for w in g["waves"].values())
    ref_pt, out_pt = str(tmp_path / "ref.pt"), str(tmp_path / "bridge.pt")
    torch.save({"model": _RefModel(g)}, ref_pt)
    tools = os.path.join(ROOT, "tools")
    sys.path.insert(0, tools)
    try:
        import export_reference_weights as ex
    finally:
        sys.path.remove(tools)
    ex.export(ref_pt, out_pt)
    ck = torch.load(out_pt, weights_only=True)
    rows = ck["yaml"]["backbone"] + ck["yaml"]["head"]
    for i in g["waves"]:
        assert rows[int(i)][3][-1] == {"wave": "db2", "use_ds": True}, i
    assert all(not (r[3] and isinstance(r[3][-1], dict)) for j, r in enumerate(rows) if str(j) not in g["waves"])
    y = E.YOLO(out_pt)
    for i in g["waves"]:
        w = y.model.model[int(i)].wave
        assert w.dwt.wave_name == "db2" and type(w.f_h).__name__ == "DSConv"
    got = y.model.state_dict()
    assert set(got) == set(ck["state_dict"])
    for k, v in ck["state_dict"].items():
        assert torch.equal(got[k], v), k
