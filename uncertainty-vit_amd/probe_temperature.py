"""Post-hoc temperature scaling for every probe head (csrc/tscale.hip): a mixin of LinearProbe."""
import contextlib
import math

import torch

from . import native
from .native import check, cur_stream, lib, ptr
from .probe_util import grown, labelled_batches, workspace

TS_MAX_N = 1 << 20           # csrc/tscale.hip: 1 <= N <= 2^20 calibration samples, K >= 2
TS_T_MIN, TS_T_MAX, TS_TOL, TS_MAX_ITER = 0.01, 100.0, 1e-7, 16
TS_STATUS = ("converged", "clamped at T_max", "clamped at T_min", "iteration limit")     # status 0 .. 3 of uvit_op_ts_fit


class TemperatureMixin:
    def _ts_fit(self, logits, ld, labels, N, t_min, t_max, tol, max_iter):
        """uvit_op_ts_fit on the current stream: the (8,) float64 device table."""
        K = self.num_classes
        ws = workspace(self, "_ts_ws", logits.device, lib().uvit_op_ts_ws_bytes, N, K)
        out = torch.zeros(8, dtype=torch.float64, device=logits.device)
        check(lib().uvit_op_ts_fit(ptr(logits), int(ld), ptr(labels), N, K, float(t_min), float(t_max), float(tol), int(max_iter), ptr(out),
                                   ptr(ws), ws.numel(), cur_stream()), "uvit_op_ts_fit")
        return out

    def temperature_batch(self, logits, labels, t_min=TS_T_MIN, t_max=TS_T_MAX, tol=TS_TOL, max_iter=TS_MAX_ITER):
        """The temperature T that minimises the mean NLL of softmax(logits / T) over caller-supplied GPU logits (N, K) fp32, N <= 2^20,
        with int64 labels (N,): the (8,) float64 device table {T, s = 1 / T, NLL at T = 1, NLL at T, dNLL/ds at s, passes used, status,
        rows left out} of uvit_op_ts_fit (include/uvit.h; status 0 converged, 1 clamped at t_max, 2 clamped at t_min, 3 max_iter passes
        used up).  Nothing synchronises with the host, and the probe's own temperature is not touched."""
        N = self._check_logits(logits, "N")
        if not 1 <= N <= TS_MAX_N:
            raise native.UvitError(f"the temperature fit takes 1 .. {TS_MAX_N} samples, got {N}")
        return self._ts_fit(logits, self.num_classes, self._labels(labels, N), N, t_min, t_max, tol, max_iter)

    def fit_temperature(self, loader, t_min=TS_T_MIN, t_max=TS_T_MAX, tol=TS_TOL, max_iter=TS_MAX_ITER):
        """Fit the temperature on a calibration loader (items as evaluate()'s): every batch goes through the forward and the
        _logits_into of evaluate(), its logits and labels into a device store grown geometrically (at most 2^20 samples), then one
        uvit_op_ts_fit over the store.  The table stays on the device for evaluate(temperature=True) and is read once:
        {"T", "nll_before" (at T = 1), "nll_after", "grad" (dNLL/ds at the result), "iterations", "status", "n", "n_skipped" (rows with
        a non-finite logit)}.  The fit sees the combined logits of an ensemble and the logits a GP or heteroscedastic evaluation sees."""
        K, store, n = self.num_classes, None, 0
        for images, labels, B in labelled_batches(self, loader):
            store = grown(store, n, n + B, TS_MAX_N, f"the temperature fit takes at most {TS_MAX_N} samples, the loader holds more",
                          (((None, K), torch.float32, 0), ((None,), torch.int64, 0)), images.device)
            self._logits_into(B)
            store[0][n:n + B].copy_(self._logits[:B])
            store[1][n:n + B].copy_(labels)
            n += B
        if not n:
            raise native.UvitError("the temperature fit needs at least one calibration sample")
        table = self._ts_fit(store[0], K, store[1], n, t_min, t_max, tol, max_iter)
        t = table.cpu().tolist()                                                         # the one read
        self._ts, self._ts_table = (t[0], t[1]), table
        nan = math.isnan(t[6])
        return {"T": t[0], "nll_before": t[2], "nll_after": t[3], "grad": t[4], "iterations": -1 if nan else int(t[5]),
                "status": -1 if nan else int(t[6]), "n": n, "n_skipped": -1 if nan else int(t[7])}

    def set_temperature(self, T):
        """Use the temperature T (a positive finite number) in evaluate(temperature=True); None forgets it.  Not a parameter and not
        a buffer: state_dict() and the checkpoints keep their keys."""
        if T is None:
            self._ts = self._ts_table = None
            return
        T = float(T)
        if not 0.0 < T < math.inf:
            raise ValueError(f"the temperature must be positive and finite, got {T}")
        self._ts, self._ts_table = (T, 1.0 / T), None

    @property
    def post_hoc_temperature(self):
        """The fitted or set post-hoc temperature, None when there is none."""
        return self._ts[0] if self._ts is not None else None

    @property
    def temperature(self):
        """post_hoc_temperature (HetProbe keeps its own `temperature`, the softmax temperature of the Monte-Carlo samples: read
        `post_hoc_temperature` there)."""
        return self.post_hoc_temperature

    @staticmethod
    def _ts_make_table(T, s, device):
        nan = float("nan")
        return torch.tensor([T, s, nan, nan, nan, 0.0, 0.0, 0.0], dtype=torch.float64).to(device)

    def _ts_begin(self, temperature):
        """(device table, host T) of evaluate(temperature=...): None leaves the evaluation as it is."""
        if temperature is None or temperature is False:
            return None, None
        self._need_gpu("the linear probe runs")
        dev = self._arena.device
        if temperature is True:
            if self._ts is None:
                raise native.UvitError("evaluate(temperature=True) needs fit_temperature() or set_temperature() first")
            if self._ts_table is None or self._ts_table.device != dev:
                self._ts_table = self._ts_make_table(self._ts[0], self._ts[1], dev)
            return self._ts_table, self._ts[0]
        T = float(temperature)
        if not 0.0 < T < math.inf:
            raise ValueError(f"the temperature must be positive and finite, got {temperature}")
        return self._ts_make_table(T, 1.0 / T, dev), T

    @contextlib.contextmanager
    def _ts_scope(self, temperature):
        """The temperature of evaluate(temperature=...) in force (self._ts_on) for the batches of one loop; gives the host T."""
        self._ts_on, value = self._ts_begin(temperature)
        try:
            yield value
        finally:
            self._ts_on = None

    def _ts_apply(self, B):
        """Inside evaluate(temperature=...): self._logits[:B] <- (float)((double) z * s), in place, directly behind _logits_into."""
        if self._ts_on is not None:
            K = self.num_classes
            check(lib().uvit_op_ts_scale(ptr(self._logits), ptr(self._logits), K, K, ptr(self._ts_on), B, K, cur_stream()), "uvit_op_ts_scale")
