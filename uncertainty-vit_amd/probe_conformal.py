"""Split conformal prediction sets for every probe head (csrc/conformal.hip): a mixin of LinearProbe."""
import ctypes as C
import math

import torch

from . import native
from .native import check, cur_stream, lib, ptr
from .probe_util import grown, labelled_batches, workspace, ws_size

CP_MAX_N, CP_MAX_K, CP_MAX_A, CP_TABLE = 1 << 20, 4096, 8, 16      # csrc/conformal.hip: rows, classes, levels, doubles per table row
CP_KINDS = {"lac": 0, "aps": 1, "raps": 2}                         # the `kind` of uvit_op_cp_scores / uvit_op_cp_sets


class ConformalMixin:
    @staticmethod
    def _cp_settings(alpha, score, lam, kreg):
        """([alpha, ...], kind, lam, kreg) checked on the host; lam and kreg belong to raps and are 0 for the other two scores."""
        alphas = [float(a) for a in (alpha if isinstance(alpha, (list, tuple)) else [alpha])]
        if not 1 <= len(alphas) <= CP_MAX_A or not all(0.0 < a < 1.0 for a in alphas):
            raise native.UvitError(f"alpha must be 1 .. {CP_MAX_A} numbers in (0, 1), got {alpha}")
        if score not in CP_KINDS:
            raise native.UvitError(f"score must be one of {list(CP_KINDS)}, got {score!r}")
        lam, kreg = (float(lam), int(kreg)) if score == "raps" else (0.0, 0)
        if not 0.0 <= lam < math.inf or kreg < 0:
            raise native.UvitError(f"raps needs lam >= 0 and kreg >= 0, got {lam}, {kreg}")
        return alphas, score, lam, kreg

    def _cp_check(self, logits, labels, u, limit=CP_MAX_N):
        """Caller-supplied logits (N, K) fp32, labels (N,) int64 and u (N,) fp32 or None, all on the GPU; returns N."""
        N = self._check_logits(logits, "N")
        if not 1 <= N <= limit or not 2 <= self.num_classes <= CP_MAX_K:
            raise native.UvitError(f"conformal sets take 1 .. {limit} rows of 2 .. {CP_MAX_K} classes, got {N} of {self.num_classes}")
        self._labels(labels, N)
        if u is not None and (not torch.is_tensor(u) or not u.is_cuda or u.dtype != torch.float32 or u.shape != (N,) or not u.is_contiguous()):
            raise native.UvitError(f"u must be a contiguous float32 GPU tensor of shape ({N},)")
        return N

    def _cp_scores_into(self, logits, ld, labels, u, N, st, dst):
        """uvit_op_cp_scores of N rows on the current stream; `dst` is a device pointer to N doubles."""
        check(lib().uvit_op_cp_scores(ptr(logits), int(ld), ptr(labels), ptr(u), N, self.num_classes, CP_KINDS[st["score"]], st["lam"],
                                      st["kreg"], C.c_void_p(dst), cur_stream()), "uvit_op_cp_scores")

    def _cp_quantile(self, scores, N, alphas):
        """uvit_op_cp_quantile on the current stream: the (A, 16) float64 device table."""
        A = len(alphas)
        ws = workspace(self, "_cp_ws", scores.device, lib().uvit_op_cp_ws_bytes, N, A)
        table = torch.zeros(A, CP_TABLE, dtype=torch.float64, device=scores.device)
        host = (C.c_double * A)(*alphas)
        check(lib().uvit_op_cp_quantile(ptr(scores), N, host, A, ptr(table), ptr(ws), ws.numel(), cur_stream()), "uvit_op_cp_quantile")
        return table

    def _cp_counters(self, A, device):
        return torch.zeros(ws_size(lib().uvit_op_cp_counter_count, self.num_classes, A), dtype=torch.int64, device=device)

    def _cp_sets_into(self, logits, ld, labels, u, B, st, counters, sizes=None, covered=None):
        A = len(st["alpha"])
        check(lib().uvit_op_cp_sets(ptr(logits), int(ld), ptr(labels), ptr(u), B, self.num_classes, CP_KINDS[st["score"]], st["lam"], st["kreg"],
                                    ptr(st["table"]), A, ptr(counters), ptr(sizes), ptr(covered), B, cur_stream()), "uvit_op_cp_sets")

    def _cp_finish(self, st, counters):
        """The state's table with the metric slots filled from `counters` (a copy: the fitted table keeps its zeros)."""
        table = st["table"].clone()
        check(lib().uvit_op_cp_finish(ptr(counters), ptr(table), self.num_classes, len(st["alpha"]), cur_stream()), "uvit_op_cp_finish")
        return table

    @staticmethod
    def _cp_result(st, rows, n_cal):
        """fit_conformal's / conformal_calibrate's host view of the table rows {alpha, q, k, n, rows left out, status}."""
        nan = any(math.isnan(r[5]) for r in rows)
        return {"alpha": list(st["alpha"]), "qhat": [r[1] for r in rows], "k": [-1 if nan else int(r[2]) for r in rows],
                "n": -1 if nan else int(rows[0][3]), "n_skipped": -1 if nan else int(rows[0][4]),
                "status": [-1 if nan else int(r[5]) for r in rows], "score": st["score"], "lam": st["lam"], "kreg": st["kreg"],
                "randomized": st["randomized"], "seed": st["seed"], "n_rows": n_cal}

    def conformal_calibrate(self, logits, labels, alpha=0.1, score="aps", lam=0.0, kreg=0, u=None):
        """Split-conformal calibration on caller-supplied GPU logits (N, K) fp32 with int64 labels (N,) and an optional fp32 u (N,) in
        [0, 1] (None: not randomised): the label scores (uvit_op_cp_scores) and their order statistics (uvit_op_cp_quantile) for one
        alpha or a list of up to 8.  Returns the state conformal_sets() and set_conformal() take: {"table": (A, 16) float64 device table
        {alpha, qhat, k, n, rows left out, status, ...}, "scores": the (N,) float64 device column, "alpha", "score", "lam", "kreg"}.
        Nothing synchronises with the host and the probe's own state is not touched."""
        alphas, score, lam, kreg = self._cp_settings(alpha, score, lam, kreg)
        N = self._cp_check(logits, labels, u)
        st = {"alpha": alphas, "score": score, "lam": lam, "kreg": kreg, "randomized": u is not None, "seed": None}
        col = torch.zeros(N, dtype=torch.float64, device=logits.device)
        self._cp_scores_into(logits, self.num_classes, labels, u, N, st, col.data_ptr())
        st["scores"], st["table"] = col, self._cp_quantile(col, N, alphas)
        return st

    def conformal_sets(self, logits, labels, state, u=None, counters=None):
        """The sets of caller-supplied GPU logits (B, K) against a state of conformal_calibrate(): {"sizes": (A, B) int32 (-1: a row
        with a non-finite logit), "covered": (A, B) uint8, "counters": the int64 device counters (pass them in again to go on adding
        over consecutive batches), "table": the (A, 16) table with the metric slots of uvit_op_cp_finish over everything the counters
        hold}.  Nothing synchronises with the host."""
        B = self._cp_check(logits, labels, u)
        A = len(state["alpha"])
        if counters is None:
            counters = self._cp_counters(A, logits.device)
        sizes = torch.zeros(A, B, dtype=torch.int32, device=logits.device)
        covered = torch.zeros(A, B, dtype=torch.uint8, device=logits.device)
        self._cp_sets_into(logits, self.num_classes, labels, u, B, state, counters, sizes, covered)
        return {"sizes": sizes, "covered": covered, "counters": counters, "table": self._cp_finish(state, counters)}

    def set_conformal(self, state):
        """Use a state of conformal_calibrate() in evaluate_conformal(); None forgets the fitted one.  Not a parameter and not a
        buffer: state_dict() and the checkpoints keep their keys."""
        if state is not None and not (isinstance(state, dict) and {"table", "alpha", "score", "lam", "kreg"} <= set(state)):
            raise native.UvitError("set_conformal takes a state of conformal_calibrate() or None")
        self._cp = None if state is None else {"randomized": False, "seed": None, **state}

    @property
    def conformal(self):
        """The fitted or set conformal state, None when there is none."""
        return self._cp

    def _cp_u(self, B, gen, device):
        return torch.rand(B, generator=gen, device=device, dtype=torch.float32) if gen is not None else None

    def fit_conformal(self, loader, alpha=0.1, score="aps", lam=0.0, kreg=0, randomized=False, seed=0, temperature=None):
        """Calibrate conformal sets on a loader (items as evaluate()'s): every batch goes through the forward, the _logits_into and the
        post-hoc temperature of evaluate(temperature=...), uvit_op_cp_scores writes its label scores into a float64 device column grown
        geometrically (at most 2^20 entries; the logits are not kept), then one uvit_op_cp_quantile.  `randomized` draws the rows' u
        from a device generator seeded with `seed` (evaluate_conformal then draws its own from seed + 1).  The table stays on the
        device for evaluate_conformal() and is read once: {"alpha", "qhat", "k", "status" (lists in the order of `alpha`; status 0: a
        finite qhat, 1: fewer rows than the level needs, qhat = +inf and every set is full), "n", "n_skipped" (rows with a non-finite
        logit), "score", "lam", "kreg", "randomized", "seed", "n_rows"}.  An ensemble contributes its combined logits, a GP or
        heteroscedastic head the logits its evaluation sees."""
        alphas, score, lam, kreg = self._cp_settings(alpha, score, lam, kreg)
        st = {"alpha": alphas, "score": score, "lam": lam, "kreg": kreg, "randomized": bool(randomized), "seed": int(seed)}
        if not 2 <= self.num_classes <= CP_MAX_K:
            raise native.UvitError(f"conformal sets take 2 .. {CP_MAX_K} classes, the head has {self.num_classes}")
        col, n, gen = None, 0, None
        with self._ts_scope(temperature):
            for images, labels, B in labelled_batches(self, loader):
                col = grown(col, n, n + B, CP_MAX_N, f"conformal calibration takes at most {CP_MAX_N} samples, the loader holds more",
                            (((None,), torch.float64, 0),), images.device)
                if randomized and gen is None:
                    gen = torch.Generator(device=images.device).manual_seed(int(seed))
                self._logits_into(B)
                self._ts_apply(B)
                self._cp_scores_into(self._logits, self.num_classes, labels, self._cp_u(B, gen, images.device), B, st, col[0].data_ptr() + 8 * n)
                n += B
        if not n:
            raise native.UvitError("conformal calibration needs at least one calibration sample")
        st["table"] = self._cp_quantile(col[0], n, alphas)
        rows = st["table"].cpu().tolist()                                              # the one read
        self._cp = st
        st["fit"] = self._cp_result(st, rows, n)
        return dict(st["fit"])

    def evaluate_conformal(self, loader, sizes=False, temperature=None):
        """The conformal sets of an evaluation loader against the fitted or set state (an error when there is none): every batch goes
        through the forward, the _logits_into and the temperature of evaluate(temperature=...), then uvit_op_cp_sets adds it to integer
        device counters; uvit_op_cp_finish and one host read follow the last batch.  Returns {"conformal": {alpha: {"coverage", "size"
        (mean), "empty", "singleton" (shares), "max_size", "sscv", "worst_class", "n", "n_skipped", "qhat"}}}; with `sizes`, also
        "sizes": the (A, n) int32 device tensor of the set sizes in loader order (-1: a row left out), an uncertainty column for
        detection_batch()."""
        st = self._cp
        if st is None:
            raise native.UvitError("evaluate_conformal needs fit_conformal() or set_conformal() first")
        A = len(st["alpha"])
        counters, gen, kept = None, None, []
        with self._ts_scope(temperature):
            for images, labels, B in labelled_batches(self, loader):
                if counters is None:
                    counters = self._cp_counters(A, images.device)
                    if st["randomized"]:
                        gen = torch.Generator(device=images.device).manual_seed(int(st["seed"] or 0) + 1)
                out = torch.zeros(A, B, dtype=torch.int32, device=images.device) if sizes else None
                self._logits_into(B)
                self._ts_apply(B)
                self._cp_sets_into(self._logits, self.num_classes, labels, self._cp_u(B, gen, images.device), B, st, counters, out)
                if sizes:
                    kept.append(out)
        nan = float("nan")
        keys = ("coverage", "size", "empty", "singleton", "max_size", "sscv", "worst_class")
        if counters is None:
            res = {"conformal": {a: {**{k: nan for k in keys}, "n": 0, "n_skipped": 0, "qhat": nan} for a in st["alpha"]}}
        else:
            rows = self._cp_finish(st, counters).cpu().tolist()                        # the one read
            res = {"conformal": {a: {**dict(zip(keys, r[6:13])), "n": int(r[13]), "n_skipped": int(r[14]), "qhat": r[1]}
                                 for a, r in zip(st["alpha"], rows)}}
            for v in res["conformal"].values():
                if not math.isnan(v["max_size"]):
                    v["max_size"] = int(v["max_size"])
        if sizes:
            res["sizes"] = torch.cat(kept, dim=1) if kept else None
        return res
