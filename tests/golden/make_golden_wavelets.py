"""Golden vectors for general wavelet filter banks (wave=) and use_ds=True of the reference's wavelet blocks
(ultralytics/nn/modules/block.py:3582-3788).  Two steps, two interpreters:

  1. python-with-PyWavelets tests/golden/make_golden_wavelets.py --pywt
       dumps dec_lo / dec_hi of every pywt.wavelist(kind="discrete") entry with filter length <= 64 to
       tests/golden/pywt_filters.json, and the same table (plus the names that are too long) to the package's
       edge-yolo_amd/nn/wavelet_filters.json.
  2. python tests/golden/make_golden_wavelets.py
       imports the REAL reference (the _ref_import recipe) with a pywt stand-in whose Wavelet(name) serves
       pywt_filters.json, and records reference outputs on synthetic weights / inputs (synthdata.py) to
       tests/golden/wavelets_ops.npz, wavelets_n_64.npz and wavelets_n_256.npz.
Runs only where the reference exists; the GPU box never runs this.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "pywt_filters.json")
PRODUCT = os.path.join(ROOT, "edge-yolo_amd", "nn", "wavelet_filters.json")
MAX_LEN = 64


def dump_pywt():
    import pywt
    table, too_long = {}, {}
    for name in pywt.wavelist(kind="discrete"):
        w = pywt.Wavelet(name)
        if w.dec_len > MAX_LEN:
            too_long[name] = int(w.dec_len)
        else:
            table[name] = dict(dec_lo=[float(v) for v in w.dec_lo], dec_hi=[float(v) for v in w.dec_hi])
    json.dump(dict(pywt_version=pywt.__version__, filters=table), open(FIXTURE, "w"), indent=0)
    json.dump(dict(source=f"PyWavelets {pywt.__version__}: pywt.Wavelet(name).dec_lo / dec_hi, kind='discrete', length <= {MAX_LEN}",
                   filters=table, too_long=too_long), open(PRODUCT, "w"), indent=0)
    print(len(table), "filters;", len(too_long), "too long:", sorted(too_long))


def reference_goldens():
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    import types
    import _ref_import
    _ref_import.setup()
    table = json.load(open(FIXTURE))["filters"]
    pywt = types.ModuleType("pywt")

    class Wavelet:  # serves the recorded PyWavelets coefficients
        def __init__(self, name):
            f = table[name]
            self.name, self.dec_lo, self.dec_hi = name, list(f["dec_lo"]), list(f["dec_hi"])
            self.dec_len = len(self.dec_lo)

    pywt.Wavelet = Wavelet
    sys.modules["pywt"] = pywt

    import numpy as np
    import torch
    import synthdata as synth
    from ultralytics.nn.tasks import DetectionModel
    from ultralytics.nn.modules import block as rb
    torch.set_grad_enabled(False)

    def filled(mod, prefix):
        mod.eval()
        for mm in mod.modules():
            if isinstance(mm, torch.nn.BatchNorm2d):
                mm.eps = 1e-3  # initialize_weights, torch_utils.py:416
        mod.load_state_dict({k: synth.synth_tensor(prefix + "." + k, tuple(v.shape)) for k, v in mod.state_dict().items()})
        return mod

    d = {}
    # _PywtDWT2D: even, odd and the smallest legal map (pad = H - 1) per wavelet; inputs stored alongside
    for name in ("haar", "db2", "sym4", "coif1", "bior2.2", "rbio3.3", "db10", "dmey"):
        dwt = rb._PywtDWT2D(name)
        pad = dwt.pad_each_side
        e = max(pad + 2 + (pad % 2), 4)
        for tag, (h, w) in (("even", (e, e + 2)), ("odd", (e + 1, e + 3)), ("min", (max(pad + 1, 2), max(pad + 1, 2) + 1))):
            x = synth.synth_images(2, h, w, c=3) * 2 - 1
            d[f"dwt_{name}_{tag}_x"] = x
            d[f"dwt_{name}_{tag}"] = torch.cat(dwt(x), 1)  # [LL | LH | HL | HH] per channel block of c
        try:  # F.pad(mode="reflect") refuses pad >= H
            dwt(torch.zeros(1, 1, max(pad, 1), pad + 4))
            d[f"dwt_{name}_raises_at_pad"] = np.int64(0)
        except RuntimeError:
            d[f"dwt_{name}_raises_at_pad"] = np.int64(1)
    # _WaveletEnhancer (block.py:3645-3710), mirroring ops_small's enh_even / enh_odd
    for c in (16, 32):
        for ds in (False, True):
            for name in ("db2", "sym4", "coif1"):
                tag = f"enh{c}_{name}_{'ds' if ds else 'conv'}"
                enh = filled(rb._WaveletEnhancer(c, use_ds=ds, wave=name), tag)
                d[tag + "_even"] = enh(synth.synth_images(2, 10, 14, c=c) - 0.5)
                d[tag + "_odd"] = enh(synth.synth_images(1, 9, 13, c=c) - 0.5)
    d["enh_ds_keys"] = np.array(sorted(rb._WaveletEnhancer(16, use_ds=True, wave="db2").state_dict()))
    # DSC3K2_Wavelet, n = 2, non-Haar wave + use_ds (block.py:3749-3788)
    for dsc3k in (False, True):
        tag = f"dsc3k2w_sym4_ds_{int(dsc3k)}"
        m = filled(rb.DSC3K2_Wavelet(32, 64, 2, dsc3k, wave="sym4", use_ds=True), tag)
        d[tag] = m(synth.synth_images(2, 12, 16, c=32) - 0.5)
    np.savez_compressed(os.path.join(HERE, "wavelets_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print("wavelets_ops", len(d))

    # whole EdgeLine-n with every enhancer replaced by _WaveletEnhancer(c, use_ds=True, wave=name)
    def model(name, b, hw, out):
        m = DetectionModel("yolo11n-test.yaml", ch=3, nc=80, verbose=False).eval()
        layers = []
        for layer in m.model:
            if isinstance(layer, rb.DSC3K2_Wavelet):
                layer.wave = rb._WaveletEnhancer(layer.c, use_ds=True, wave=name)
                for mm in layer.wave.modules():
                    if isinstance(mm, torch.nn.BatchNorm2d):
                        mm.eps = 1e-3  # as initialize_weights (torch_utils.py:416) sets it for every module the model was built with
                layers.append(layer.i)
        m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
        m.fuse(verbose=False)
        m.eval()
        y, raw = m(synth.synth_images(b, hw, hw))
        g = {f"raw{i}": r.numpy() for i, r in enumerate(raw)}
        g["wave_layers"] = np.array(layers)
        np.savez_compressed(os.path.join(HERE, out), **g)
        print(out, [r.shape for r in raw])

    model("db2", 2, 64, "wavelets_n_64.npz")
    model("sym4", 1, 256, "wavelets_n_256.npz")
    # what the reference model of the export test holds: DetectionModel('yolo11n-test.yaml') with db2 + use_ds enhancers
    m = DetectionModel("yolo11n-test.yaml", ch=3, nc=80, verbose=False)
    waves = {}
    for layer in m.model:
        if isinstance(layer, rb.DSC3K2_Wavelet):
            layer.wave = rb._WaveletEnhancer(layer.c, use_ds=True, wave="db2")
            waves[layer.i] = dict(c=layer.c, wave_name=layer.wave.dwt.wave_name, mode=layer.wave.dwt.mode, f_h=type(layer.wave.f_h).__name__)
    sd = m.state_dict()
    json.dump(dict(yaml=dict(m.yaml), waves=waves, state_shapes={k: list(v.shape) for k, v in sd.items()}),
              open(os.path.join(HERE, "ref_checkpoint_n_db2_ds.json"), "w"), indent=0)


if __name__ == "__main__":
    dump_pywt() if "--pywt" in sys.argv else reference_goldens()
