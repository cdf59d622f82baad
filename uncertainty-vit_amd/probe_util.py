"""What every probe family needs, written once: the two batch loops, the workspace query, the growing device store, the mean of a
per-sample column, and the part of a feature-side score (probe_density.py, probe_neighbours.py, probe_vim.py) that does not depend on the score."""
import math

import torch

from . import native
from .native import check


def labelled_batches(probe, loader):
    """(images, labels, B) of a loader of (images, labels) or ((images, mask), labels): the batch's features are in probe._feat[:B]
    (probe._features), the labels on the device and checked (probe._labels)."""
    for item in loader:
        images, labels = item
        if isinstance(images, (tuple, list)):
            images = images[0]
        B = probe._features(images)
        if torch.is_tensor(labels) and not labels.is_cuda:
            labels = labels.to(images.device, non_blocking=True)
        yield images, probe._labels(labels, B), B


def image_batches(probe, loader):
    """(images, B) of a loader of images, (images, labels) or ((images, mask), labels); labels, if any, are ignored."""
    for item in loader:
        images = item
        while isinstance(images, (tuple, list)):
            images = images[0]
        yield images, probe._features(images)


def ws_size(fn, *args, name=None):
    """What a `*_ws_bytes` (or counter-count) query of the library answers; a negative answer is its error code."""
    n = fn(*args)
    if n < 0:
        check(int(n), name or fn.__name__)
    return int(n)


def workspace(owner, slot, device, fn, *args, name=None):
    """The uint8 device tensor `owner.<slot>` with at least fn(*args) bytes on `device`: grown, never shrunk."""
    need = ws_size(fn, *args, name=name)
    ws = getattr(owner, slot, None)
    if ws is None or ws.numel() < need or ws.device != device:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        setattr(owner, slot, ws)
    return ws


def grown(tensors, n, need, limit, message, specs, device, hint=0):
    """Device tensors with room for `need` samples, of which the first `n` are kept.  `specs` holds (shape, dtype, fill) per tensor,
    the shape with None at the sample axis; `tensors` is what grown() returned before, or None.  More than `limit` samples raise
    `message`; the capacity grows geometrically, from `hint` where the caller knows the final size."""
    if need > limit:
        raise native.UvitError(message)
    axes = [shape.index(None) for shape, _, _ in specs]
    cap = tensors[0].shape[axes[0]] if tensors is not None else 0
    if need <= cap:
        return tensors
    cap, out = min(limit, max(need, 2 * cap, hint, 1024)), []
    for i, ((shape, dtype, fill), axis) in enumerate(zip(specs, axes)):
        shape = [cap if s is None else s for s in shape]
        t = torch.full(shape, fill, dtype=dtype, device=device) if fill else torch.zeros(shape, dtype=dtype, device=device)
        if n:
            t.narrow(axis, 0, n).copy_(tensors[i].narrow(axis, 0, n))
        out.append(t)
    return tuple(out)


def column_mean(slabs, skip_nan=False):
    """The float64 mean of a column kept as per-batch device slabs: one read; NaN without a row (with `skip_nan`: a row that is not
    NaN)."""
    vals = torch.cat(slabs).cpu().tolist() if slabs else []
    if skip_nan:
        vals = [v for v in vals if not math.isnan(v)]
    return math.fsum(vals) / len(vals) if vals else float("nan")


class FeatureScore:
    """An out-of-distribution score of the probe's features that a fit over a labelled set makes available: its state (None until a
    fit or a load), the detection columns it appends while it has one, and its part of evaluate(detection=True).  A subclass has
    `columns`, `stat_prefix`, `device_keys` (the state's device tensors), `into()` and `eval_batch()`."""

    def __init__(self, probe):
        self.probe, self.state, self.batch = probe, None, 0

    def moved(self, device):
        """The probe went to `device`: the state follows, the batch-sized buffers are allocated again."""
        self.batch = 0
        if self.state is not None:
            for key in self.device_keys:
                self.state[key] = self.state[key].to(device)

    @property
    def info(self):
        return dict(self.state["info"]) if self.state is not None else None

    def forget(self):
        self.state = None
        self.probe._det_refresh()

    def need(self, who, verb="needs"):
        """The state; without one, `who` is refused."""
        if self.state is None:
            raise native.UvitError(f"{who} {verb} {self.fitters} first")
        return self.state

    def eval_stats(self, ev, n):
        """The score's two entries of evaluate()'s result: the mean of its first column over the evaluation rows that are not NaN and
        its classifier's accuracy in percent; read with the counters, after the last batch."""
        mean, acc = f"{self.stat_prefix}_mean", f"{self.stat_prefix}_acc1"
        if not n:
            return {mean: float("nan"), acc: float("nan")}
        return {mean: column_mean(ev["slabs"], skip_nan=True), acc: 100.0 * int(ev["correct"].cpu()) / n}
