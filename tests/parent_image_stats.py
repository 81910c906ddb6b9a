"""DetectionValidator._image_stats as it stood before the confusion_matrix / device_match keywords existed (no `tps`, no `host_cm`), kept as
a baseline for the tests that say "with both keywords off nothing changes": a regression inside today's loop shows against this copy."""
import numpy as np

from edge_yolo_amd.engine.validator import _np


def image_stats(self, rows, batch, pbatches=None, **more_tp):
    for si, pred in enumerate(rows):
        self.seen += 1
        pred = _np(pred).astype(np.float32)
        pred = pred.reshape(-1, pred.shape[-1] if pred.ndim == 2 else 6)
        npr = pred.shape[0]
        stat = dict(conf=np.zeros(0, np.float32), pred_cls=np.zeros(0, np.float32), **{k: np.zeros((npr, self.niou), bool) for k in ("tp", *more_tp)})
        pbatch = self._prepare_batch(si, batch) if pbatches is None else pbatches[si]
        cls = pbatch["cls"]
        stat["target_cls"] = cls
        stat["target_img"] = np.unique(cls)
        if npr == 0:
            if len(cls):
                for k in self.stats:
                    self.stats[k].append(stat[k])
            continue
        if self.single_cls:
            pred = pred.copy()
            pred[:, 5] = 0
        predn = self._box_rows(pred, pbatch)
        stat["conf"], stat["pred_cls"] = predn[:, 4], predn[:, 5]
        if len(cls):
            stat["tp"] = self._box_tp(si, predn, pbatch)
            for k, f in more_tp.items():
                stat[k] = f(si, predn, pbatch)
        for k in self.stats:
            self.stats[k].append(stat[k])
