"""Feature density of the probe: Mahalanobis and relative Mahalanobis scores (csrc/maha.hip).  FeatureDensity
is the score (probe_util.FeatureScore); DensityMethods are LinearProbe's public methods for it."""
import ctypes as C
import math

import torch

from . import native
from .native import check, cur_stream, lib, ptr
from .probe_util import FeatureScore, labelled_batches, workspace

MAHA_MAX_C, MAHA_MAX_K = 2048, 4096          # csrc/maha.hip: C % 4 == 0, 4 <= C <= 2048, 2 <= K <= 4096, 1 <= B <= 65535
MAHA_COLUMNS = ("maha", "rmaha")             # the detection columns a fitted density appends to the class's
MAHA_SHRINKAGE = 1e-3                        # an option's default, not a measured optimum
SUM_KEYS = ("S", "class_sum", "total_sum", "class_count", "sums")


def _shrinkage(shrinkage):
    rho = float(shrinkage)
    if not 0.0 < rho < math.inf:
        raise native.UvitError(f"the shrinkage must be positive and finite, got {shrinkage}")
    return rho


class FeatureDensity(FeatureScore):
    """State: the host float64 sums (SUM_KEYS), the device float64 W, W0, Wmu, Wmu0 and count_dev, and `info`."""
    columns, stat_prefix, device_keys = MAHA_COLUMNS, "maha", ("W", "W0", "Wmu", "Wmu0", "count_dev")
    fitters = "fit_density() or load_density_state()"

    def install(self, S, class_sum, total_sum, class_count, sums, shrinkage):
        """Host float64 sums -> the two shrunk covariances, their Cholesky factors, the whitened means and the uploads."""
        rho = _shrinkage(shrinkage)
        K, Cd, F64 = self.probe.num_classes, self.probe.embed_dim, torch.float64
        if Cd < 4 or Cd % 4 or Cd > MAHA_MAX_C or not 2 <= K <= MAHA_MAX_K:
            raise native.UvitError(f"the Mahalanobis ops take an embed dim that is a multiple of 4 in [4, {MAHA_MAX_C}] and 2 .. {MAHA_MAX_K} "
                                   f"classes, got {Cd} and {K}")
        S, class_sum, total_sum, class_count, sums = (torch.as_tensor(t, dtype=F64).cpu().contiguous()
                                                      for t in (S, class_sum, total_sum, class_count, sums))
        if (tuple(S.shape), tuple(class_sum.shape), tuple(total_sum.shape), tuple(class_count.shape), tuple(sums.shape)) != \
                ((Cd, Cd), (K, Cd), (Cd,), (K,), (2,)):
            raise native.UvitError(f"the density state belongs to another probe: its sums must have shapes ({Cd}, {Cd}), ({K}, {Cd}), "
                                   f"({Cd},), ({K},) and (2,)")
        n, skipped = float(sums[0]), float(sums[1])
        if not n >= 2:
            raise native.UvitError("the density fit needs at least two usable rows (finite features, a label inside [0, K))")
        mu = class_sum / class_count.clamp_min(1.0)[:, None]                 # an empty class: a zero row, never chosen
        mu0 = total_sum / n
        sigma = (S - class_sum.T @ mu) / n                                   # sum_k n_k mu_k mu_k^T = class_sum^T mu
        sigma = 0.5 * (sigma + sigma.T)
        sigma0 = S / n - torch.outer(mu0, mu0)
        eye = torch.eye(Cd, dtype=F64)
        fac = []
        for m in (sigma, sigma0):
            reg = m + rho * (float(torch.trace(m)) / Cd) * eye
            L, info = torch.linalg.cholesky_ex(reg)
            if int(info) != 0 or not bool(torch.isfinite(L).all()):
                raise native.UvitError("the density fit failed: a shrunk covariance is not positive definite (constant or non-finite "
                                       "features?); try a larger shrinkage")
            fac.append((torch.linalg.solve_triangular(L, eye, upper=False).tril(), 2.0 * float(torch.log(torch.diagonal(L)).sum())))
        (W, logdet), (W0, logdet0) = fac
        dev = self.probe._arena.device
        up = lambda t: t.contiguous().to(dev)                                # noqa: E731
        self.state = {"S": S, "class_sum": class_sum, "total_sum": total_sum, "class_count": class_count, "sums": sums,
                      "W": up(W), "W0": up(W0), "Wmu": up(mu @ W.T), "Wmu0": up(W0 @ mu0), "count_dev": up(class_count),
                      "info": {"n": int(n), "skipped": int(skipped), "classes": K, "empty_classes": int((class_count <= 0).sum()),
                               "shrinkage": rho, "logdet": logdet, "logdet0": logdet0}}
        self.probe._det_refresh()
        return self.info

    def accumulate(self, loader):
        """One pass of uvit_op_maha_accumulate over a labelled loader and one read: the host float64 (S, class_sum, total_sum,
        class_count, sums), None for a loader without a batch.  The density's fit and the first pass of the ViM fit (probe_vim.py)."""
        p = self.probe
        K, Cd, acc = p.num_classes, p.embed_dim, None
        o_cs, o_ts, o_cc, o_sums = Cd * Cd, Cd * Cd + K * Cd, Cd * Cd + K * Cd + Cd, Cd * Cd + K * Cd + Cd + K
        for images, labels, B in labelled_batches(p, loader):
            if acc is None:
                acc = torch.zeros(o_sums + 2, dtype=torch.float64, device=images.device)     # S | class sums | total | counts | sums
            ws = workspace(self, "fit_ws", images.device, lib().uvit_op_maha_accumulate_ws_bytes, B, Cd, K)
            at = lambda off: C.c_void_p(acc.data_ptr() + 8 * off)                             # noqa: E731
            check(lib().uvit_op_maha_accumulate(ptr(p._feat), ptr(labels), at(0), at(o_cs), at(o_ts), at(o_cc), at(o_sums), ptr(ws),
                                                ws.numel(), B, Cd, K, cur_stream()), "uvit_op_maha_accumulate")
        self.fit_ws = None                                                                    # the fit's workspace is not kept
        if acc is None:
            return None
        host = acc.cpu()                                                                      # the one read
        return host[:o_cs].view(Cd, Cd), host[o_cs:o_ts].view(K, Cd), host[o_ts:o_cc], host[o_cc:o_sums], host[o_sums:o_sums + 2]

    def fit(self, loader, shrinkage):
        rho = _shrinkage(shrinkage)
        sums = self.accumulate(loader)
        if sums is None:
            raise native.UvitError("the density fit needs at least two labelled samples")
        return self.install(*sums, rho)

    def buffers_for(self, B):
        p = self.probe
        if B > self.batch:
            dev = p._arena.device
            workspace(self, "ws", dev, lib().uvit_op_maha_scores_ws_bytes, B, p.embed_dim, p.num_classes)
            self.col, self.rcol = (torch.zeros(B, dtype=torch.float32, device=dev) for _ in range(2))
            self.pred = torch.zeros(B, dtype=torch.int32, device=dev)
            self.batch = B
        if self.ws.device != self.state["W"].device:
            raise native.UvitError("the density and the probe are on different devices")

    def into(self, feat, B, dist=None, labels=None, correct=None):
        """uvit_op_maha_scores of feat[:B] on the current stream into self.col, self.rcol and self.pred."""
        st, p = self.need("the Mahalanobis scores", "need"), self.probe
        p._need_gpu("the Mahalanobis scores run")
        self.buffers_for(B)
        K = p.num_classes
        check(lib().uvit_op_maha_scores(ptr(feat), ptr(st["W"]), ptr(st["W0"]), ptr(st["Wmu"]), ptr(st["Wmu0"]), ptr(st["count_dev"]),
                                        ptr(self.col), ptr(self.rcol), ptr(self.pred), ptr(dist), K, ptr(labels), ptr(correct),
                                        ptr(self.ws), self.ws.numel(), B, p.embed_dim, K, cur_stream()), "uvit_op_maha_scores")

    def result(self, feat, B, distances):
        dist = torch.zeros(B, self.probe.num_classes, dtype=torch.float64, device=feat.device) if distances else None
        self.into(feat, B, dist)
        out = {"maha": self.col[:B].clone(), "rmaha": self.rcol[:B].clone(), "pred": self.pred[:B].clone()}
        if distances:
            out["dist"] = dist
        return out

    def eval_batch(self, B, labels, ev):
        """Inside evaluate(detection=True): the two columns of the probe's features into the store (behind _det_reserve, in front of
        _det_rows).  The evaluation set's rows (labels given) are also counted against their labels and kept for the mean."""
        self.into(self.probe._feat, B, None, labels, ev["correct"] if labels is not None else None)
        self.probe._own_column("maha", self.col, B, ev["slabs"])
        self.probe._own_column("rmaha", self.rcol, B, None)


class DensityMethods:
    """LinearProbe's methods for its FeatureDensity, `self._density`."""
    _maha = property(lambda self: self._density.state, doc="the density's state dict, None when there is none")

    def fit_density(self, loader, shrinkage=MAHA_SHRINKAGE):
        """Class-conditional Gaussians with one tied covariance, and one background Gaussian, on the probe's features: one pass over a
        labelled loader (items as evaluate()'s) of the encoder forward, pool + norm and uvit_op_maha_accumulate into device
        accumulators, one read of the sums, then the host's two covariances, their shrinkage Sigma + shrinkage tr(Sigma) / C I and
        Cholesky factors in float64 (torch.linalg on the CPU) and the upload of W = L^-1, W0 = L0^-1 and the whitened means.  The head
        takes no part: any trained or untrained head gets the columns.  Returns {n, skipped (rows with a non-finite feature or a label
        outside [0, K)), classes, empty_classes, shrinkage, logdet, logdet0 (log-determinants of the two shrunk covariances)}."""
        return self._density.fit(loader, shrinkage)

    def set_density(self, state):
        """None forgets the density (the detection columns are the class's again); a dict of density_state_dict() is loaded."""
        if state is not None:
            return self.load_density_state(state)
        self._density.forget()

    @property
    def density(self):
        """{n, skipped, classes, empty_classes, shrinkage, logdet, logdet0} of the density in use, None when there is none."""
        return self._density.info

    def set_density_shrinkage(self, shrinkage):
        """Another shrinkage for the density in use: the host factorises again from the kept sums, the data are not read."""
        st = self._density.need("set_density_shrinkage")
        return self._density.install(*(st[k] for k in SUM_KEYS), shrinkage)

    def density_state_dict(self):
        """What a density is made of, on the host: the float64 sums S, class_sum, total_sum, class_count, sums = {rows used, rows
        skipped} and the shrinkage.  Not part of state_dict(): neither a parameter nor a buffer."""
        st = self._density.need("density_state_dict")
        return {**{k: st[k].clone() for k in SUM_KEYS}, "shrinkage": st["info"]["shrinkage"]}

    def load_density_state(self, sd):
        """Install a saved density (density_state_dict()); one of another embed dim or class count is refused."""
        keys = SUM_KEYS + ("shrinkage",)
        if not (isinstance(sd, dict) and set(keys) <= set(sd)):
            raise native.UvitError("load_density_state takes a dict of density_state_dict()")
        return self._density.install(*(sd[k] for k in keys))

    def feature_scores(self, images, distances=False):
        """{"maha", "rmaha" (B) fp32, "pred" (B) int32} of the images' features against the density in use, device tensors; with
        `distances`, also "dist" (B, K) float64, the squared distance to every class mean.  maha = the smallest squared Mahalanobis
        distance to a class mean under the tied covariance, pred = that class (the nearest class mean), rmaha = maha minus the squared
        distance to the background Gaussian; larger = more out of distribution.  A row with a non-finite feature: NaN, NaN, -1."""
        self._density.need("feature_scores")
        B = self._features(images)
        return self._density.result(self._feat, B, distances)

    def density_batch(self, feat, distances=False):
        """feature_scores() of caller-supplied GPU features (B, C) fp32; nothing synchronises with the host."""
        return self._density.result(feat, self._check_feat(feat), distances)
