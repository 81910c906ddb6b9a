#!/usr/bin/env python
"""Weight bridge, REFERENCE side: turn a checkpoint written by the reference trainer (a pickled module object,
engine/trainer.py:513-546; read back by nn/tasks.py:815-955) into the tensor-only format `edge_yolo_amd.YOLO(path)` loads with
`torch.load(weights_only=True)`:  {"yaml": <model yaml dict>, "nc": int, "fused": bool, "state_dict": {reference keys: fp32 tensors}}.
A YOLO-World checkpoint also gets its text embeddings (state_dict key `txt_feats`) and a `names` list (`edge_yolo_amd.YOLOWorld(path)`).

Run it where the reference package (`ultralytics`, this fork) is importable -- unpickling a reference checkpoint executes its module
code, which is why edge-yolo_amd never does it:

    python tools/export_reference_weights.py runs/detect/train/weights/best.pt edgeline_gc10.pt
    >>> from edge_yolo_amd import YOLO; YOLO("edgeline_gc10.pt").predict(batch, half=True)
"""
import sys

import torch


def _record_wavelet_kwargs(model, cfg):
    """The DWT filter of a reference _PywtDWT2D is a non-persistent buffer, and wave= / use_ds= are constructor kwargs its YAML
    cannot express: a state_dict alone would load as a Haar / dense-f_h model.  Each DSC3K2_Wavelet layer whose enhancer is not
    the default gets a trailing {wave:, use_ds:, mode:} mapping in its yaml args (edge-yolo_amd's parse_model reads it)."""
    rows = None
    for layer in model.modules():
        if type(layer).__name__ != "DSC3K2_Wavelet":
            continue
        enh = layer.wave
        wave, mode = getattr(enh.dwt, "wave_name", "haar"), getattr(enh.dwt, "mode", "symmetric")
        use_ds = type(enh.f_h).__name__ == "DSConv"
        if wave == "haar" and not use_ds and mode == "symmetric":
            continue
        if rows is None:
            cfg["backbone"] = [list(r) for r in cfg["backbone"]]
            cfg["head"] = [list(r) for r in cfg["head"]]
            rows = cfg["backbone"] + cfg["head"]
        row = rows[layer.i]  # (parse_model sets .i, the layer's index in backbone + head)
        args = list(row[3])
        extra = dict(args.pop()) if args and isinstance(args[-1], dict) else {}
        extra.update(wave=wave, use_ds=use_ds)
        if mode != "symmetric":
            extra["mode"] = mode
        row[3] = args + [extra]


def export(src, dst):
    ck = torch.load(src, map_location="cpu", weights_only=False)  # a reference checkpoint: pickled nn.Module (trusted input of the reference's user)
    model = ck.get("ema") or ck["model"] if isinstance(ck, dict) else ck
    model = model.float().eval()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cfg = dict(model.yaml)  # the parsed YAML incl. 'scale', 'nc', 'ch', 'yaml_file' (tasks.py:331-337)
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}
    first_conv = next(k for k in sd if k.endswith("conv.weight"))
    fused = first_conv.replace("conv.weight", "bn.weight") not in sd  # BaseModel.fuse() deleted the BatchNorms (tasks.py:214-242)
    _record_wavelet_kwargs(model, cfg)
    extra = {}
    if type(model).__name__ == "WorldModel":  # YOLO-World: the text is a plain attribute there (tasks.py:629,651); edge-yolo_amd keeps it as the buffer `txt_feats`
        t = model.txt_feats.detach().float()
        sd["txt_feats"] = t.reshape(1, -1, t.shape[-1]).clone()
        names = getattr(model, "names", None) or {}
        extra["names"] = [str(names[i]) for i in sorted(names)] if isinstance(names, dict) else [str(n) for n in names]
    torch.save({"yaml": cfg, "nc": int(cfg["nc"]), "fused": bool(fused), "state_dict": sd, **extra}, dst)
    return len(sd), fused


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    n, fused = export(sys.argv[1], sys.argv[2])
    print(f"wrote {sys.argv[2]}: {n} tensors, fused={fused}")
