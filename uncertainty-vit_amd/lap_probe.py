"""Post-hoc last-layer Laplace approximation of a trained linear probe head: the method the reference names with its `--laplace` flag
(run_class_finetuning.py:651-653: `Laplace(model, 'classification', subset_of_weights='last_layer', hessian_structure='kron')`,
commented out and never wired in), built for the frozen encoder with one nn.Linear.

    phi = [f, 1] (D = C + 1)    z = W f + b    p = softmax(z)    theta ordered (k, c'), the C weights of class k, then its bias
    fit:      A = sum_n phi phi^T (D, D)    G = (1 / n) sum_n (diag(p) - p p^T) (K, K)    precision = G (x) A + tau I
    predict:  var_k = sum_i a_i^2 T[i, k],  a = U_A^T phi,  T[i, k] = sum_j U_G[k, j]^2 / (lam_A[i] lam_G[j] + tau)
              z~_k = z_k / sqrt(1 + (pi / 8) var_k)   (the probit link)          lap_var = var at the arg-max of z

The model is linear in the head's parameters, so the GGN is the Hessian and the Jacobian of the logits is I_K (x) phi^T: the two
Kronecker factors are exact sums over one pass of a labelled set.  They accumulate on the device (uvit_op_lap_factors), are read
once, and the two symmetric eigen-decompositions are float64 on the host (torch.linalg.eigh, as inv(P) of the GP head is formed on
the host): plumbing, once per fit.  The per-batch work -- uvit_op_lap_variance and uvit_op_lap_probit -- runs as the HIP kernels of
csrc/laplace.hip on the stream of the encoder forward, directly behind _logits_into and in front of the post-hoc temperature, so
everything LinearProbe computes from logits (evaluate, fit_temperature, fit_conformal, evaluate_conformal, evaluate_stability,
logits()) sees z~.  The head was trained with label smoothing and weight decay, so it is not the MAP of this model: the usual
post-hoc use.  There is no CPU fallback.
"""
import ctypes as C
import hashlib
import math

import numpy as np
import torch

from . import native
from .linear_probe import LinearProbe
from .native import check, cur_stream, lib, ptr
from .probe_util import labelled_batches, workspace

__all__ = ["LaplaceProbe", "marglik_grid", "log_marglik", "choose_prior_precision"]

LAP_MAX_C, LAP_MAX_K = 2048, 4096          # csrc/laplace.hip: C % 4 == 0, 4 <= C <= 2048, 2 <= K <= 4096, 1 <= B <= 65535
PROBIT_FACTOR = math.pi / 8.0              # the probit link of the Laplace literature
F64 = torch.float64


def marglik_grid():
    """The 97 log-spaced prior precisions of [1e-4, 1e8] (eight per decade) that `marglik` searches."""
    return np.logspace(-4.0, 8.0, 97)


def log_marglik(tau, nll, theta_sq, lam_a, lam_g):
    """log ml(tau) = -nll - tau |theta|^2 / 2 + K D log(tau) / 2 - sum_ij log(lam_A[i] lam_G[j] + tau) / 2, float64 on the host;
    lam_a (D) and lam_g (K) are the clamped eigenvalues of A and G."""
    lam_a, lam_g = torch.as_tensor(lam_a, dtype=F64), torch.as_tensor(lam_g, dtype=F64)
    tau = float(tau)
    logdet = float(torch.log(torch.outer(lam_a, lam_g) + tau).sum())
    return -float(nll) - 0.5 * tau * float(theta_sq) + 0.5 * lam_a.numel() * lam_g.numel() * math.log(tau) - 0.5 * logdet


def choose_prior_precision(nll, theta_sq, lam_a, lam_g):
    """(tau, log ml(tau), on_grid_edge): the arg-max of log_marglik over marglik_grid(); the first point wins ties."""
    grid = marglik_grid()
    vals = [log_marglik(t, nll, theta_sq, lam_a, lam_g) for t in grid]
    i = int(np.argmax(vals))
    return float(grid[i]), vals[i], i in (0, len(grid) - 1)


def _prior_arg(prior_precision):
    if isinstance(prior_precision, str):
        if prior_precision != "marglik":
            raise ValueError(f"prior_precision is a positive number or 'marglik', got {prior_precision!r}")
        return prior_precision
    tau = float(prior_precision)
    if not 0.0 < tau < math.inf:
        raise ValueError(f"prior_precision must be positive and finite, got {prior_precision}")
    return tau


class LaplaceProbe(LinearProbe):
    """A LinearProbe with a post-hoc Laplace fit.  state_dict() holds exactly `head.weight` and `head.bias`, so any linear
    probe-N.pth loads; the Laplace state is neither a parameter nor a buffer (laplace_state_dict / load_laplace_state carry it).
    Without a fit the probe launches and returns what a LinearProbe does, bit for bit; train_step, load_state_dict and a move to
    another device drop the fit."""

    DETECT_COLUMNS = LinearProbe.DETECT_COLUMNS + ("lap_var",)

    def __init__(self, encoder, num_classes, smoothing=0.1, init_scale=0.001):
        Cd, K = int(encoder.embed_dim), int(num_classes)
        if Cd < 4 or Cd % 4 or Cd > LAP_MAX_C or not 2 <= K <= LAP_MAX_K:
            raise ValueError(f"the Laplace ops take an embed dim that is a multiple of 4 in [4, {LAP_MAX_C}] and 2 .. {LAP_MAX_K} classes, "
                             f"got {Cd} and {K}")
        super().__init__(encoder, num_classes, smoothing=smoothing, init_scale=init_scale)
        self._lap_batch = 0
        self.set_laplace(None)

    # ---- state ----
    def set_laplace(self, state):
        """None forgets the fit; a dict of laplace_state_dict() is loaded (load_laplace_state)."""
        if state is not None:
            return self.load_laplace_state(state)
        self._lap = None
        self._det_refresh()                                    # unfitted: the columns, and so the launches, of a LinearProbe

    def _det_class_columns(self):
        return LinearProbe.DETECT_COLUMNS if self._lap is None else type(self).DETECT_COLUMNS

    @property
    def laplace(self):
        """{n, n_skipped, nll, prior_precision, log_marglik, on_grid_edge} of the fit in use, None when there is none."""
        return dict(self._lap["info"]) if self._lap is not None else None

    def _apply(self, fn, recurse=True):
        self._lap_batch = 0
        self.set_laplace(None)
        return super()._apply(fn, recurse)

    def load_state_dict(self, state_dict, strict=True, **kw):
        self.set_laplace(None)
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        """LinearProbe.train_step; the fit belongs to the head as it was and is dropped."""
        self.set_laplace(None)
        return super().train_step(images, labels, lr, weight_decay, max_norm)

    def _head_host(self):
        """The head's K (C + 1) parameters as a float32 host tensor (the arena without its padding)."""
        K, Cd = self.num_classes, self.embed_dim
        return self._arena[:K * Cd + K].detach().cpu().contiguous()

    @staticmethod
    def _head_hash(head):
        return hashlib.sha256(head.numpy().tobytes()).hexdigest()

    def _lap_buffers_for(self, B):
        if B > self._lap_batch:
            K, Cd, dev = self.num_classes, self.embed_dim, self._arena.device
            for query in (lib().uvit_op_lap_factors_ws_bytes, lib().uvit_op_lap_variance_ws_bytes):      # one workspace for both ops
                workspace(self, "_lap_ws", dev, query, B, Cd, K, name="uvit_op_lap_*_ws_bytes")
            self._lap_var = torch.zeros(B, K, dtype=F64, device=dev)
            self._lap_col = torch.zeros(B, dtype=torch.float32, device=dev)
            self._lap_batch = B

    def _install(self, A, G_sum, sums, prior, head=None):
        """Host float64 factors -> eigen-decompositions, the prior precision, the uploads and uvit_op_lap_prepare."""
        self._need_gpu("the Laplace probe runs")
        dev = self._arena.device
        K, D = self.num_classes, self.embed_dim + 1
        A, G_sum, sums = (torch.as_tensor(t, dtype=F64).cpu().contiguous() for t in (A, G_sum, sums))
        if tuple(A.shape) != (D, D) or tuple(G_sum.shape) != (K, K) or tuple(sums.shape) != (3,):
            raise native.UvitError(f"the Laplace factors must have shapes ({D}, {D}), ({K}, {K}) and (3,)")
        nll, n, skipped = (float(v) for v in sums)
        if not n >= 1:
            raise native.UvitError("the Laplace fit needs at least one usable row (finite logits, a label inside [0, K))")
        head = self._head_host() if head is None else head
        lam_a, UA = torch.linalg.eigh(A)
        lam_g, UG = torch.linalg.eigh(G_sum / n)
        lam_a, lam_g = lam_a.clamp_min(0.0), lam_g.clamp_min(0.0)       # G has the all-ones null vector: eigh returns about -1e-17 there
        up = lambda t: t.contiguous().to(dev)                           # noqa: E731
        self._lap = {"A": A, "G_sum": G_sum, "sums": sums, "lam_a": lam_a, "lam_g": lam_g, "theta_sq": float((head.double() ** 2).sum()),
                     "head_sha256": self._head_hash(head), "UA": up(UA), "UG": up(UG), "lam_a_dev": up(lam_a), "lam_g_dev": up(lam_g),
                     "T": torch.zeros(D, K, dtype=F64, device=dev),
                     "info": {"n": int(n), "n_skipped": int(skipped), "nll": nll}}
        self._det_refresh()                                             # fitted: the class's columns, lap_var among them
        return self.set_prior_precision(prior)

    def set_prior_precision(self, prior_precision):
        """Another tau for the fit in use (a positive number or 'marglik'): uvit_op_lap_prepare alone runs again, the data are not
        read.  Returns the fit's {n, n_skipped, nll, prior_precision, log_marglik, on_grid_edge}."""
        st = self._lap
        if st is None:
            raise native.UvitError("set_prior_precision needs fit_laplace() or load_laplace_state() first")
        prior = _prior_arg(prior_precision)
        nll = st["info"]["nll"]
        if prior == "marglik":
            tau, ml, edge = choose_prior_precision(nll, st["theta_sq"], st["lam_a"], st["lam_g"])
        else:
            tau, ml, edge = prior, log_marglik(prior, nll, st["theta_sq"], st["lam_a"], st["lam_g"]), False
        check(lib().uvit_op_lap_prepare(ptr(st["UG"]), ptr(st["lam_a_dev"]), ptr(st["lam_g_dev"]), C.c_double(tau), ptr(st["T"]),
                                        self.embed_dim, self.num_classes, cur_stream()), "uvit_op_lap_prepare")
        st["info"].update(prior_precision=tau, log_marglik=ml, on_grid_edge=bool(edge))
        return dict(st["info"])

    def fit_laplace(self, loader, prior_precision=1.0):
        """One pass over a labelled loader (items as evaluate()'s): encoder forward, pool + norm, the head's logits and
        uvit_op_lap_factors per batch into device accumulators; one read of A, G_sum and the sums; then the host's eigh, the prior
        precision (a positive number, or 'marglik': the arg-max of the marginal likelihood over marglik_grid()), the upload of the
        eigenvectors and eigenvalues and uvit_op_lap_prepare.  Returns {n, n_skipped (rows with a non-finite logit or a label outside
        [0, K)), nll (the sum over the n rows), prior_precision, log_marglik, on_grid_edge}."""
        prior = _prior_arg(prior_precision)
        self.set_laplace(None)
        K, Cd = self.num_classes, self.embed_dim
        D, acc = Cd + 1, None
        for images, labels, B in labelled_batches(self, loader):
            if acc is None:
                acc = torch.zeros(D * D + K * K + 4, dtype=F64, device=images.device)        # A | G_sum | sums: one allocation, one read
            self._lap_buffers_for(B)
            LinearProbe._logits_into(self, B)
            at = lambda off: C.c_void_p(acc.data_ptr() + 8 * off)                            # noqa: E731
            check(lib().uvit_op_lap_factors(ptr(self._feat), ptr(self._logits), K, ptr(labels), at(0), at(D * D), at(D * D + K * K),
                                            ptr(self._lap_ws), self._lap_ws.numel(), B, Cd, K, cur_stream()), "uvit_op_lap_factors")
        if acc is None:
            raise native.UvitError("the Laplace fit needs at least one labelled sample")
        host = acc.cpu()                                                                     # the one read
        return self._install(host[:D * D].view(D, D), host[D * D:D * D + K * K].view(K, K), host[D * D + K * K:D * D + K * K + 3], prior)

    def laplace_state_dict(self):
        """What a fit is made of, on the host: the float64 factors A and G_sum (not divided by n), sums = {nll, rows used, rows
        skipped}, the prior precision and a SHA-256 of the head's bytes."""
        st = self._lap
        if st is None:
            raise native.UvitError("laplace_state_dict needs fit_laplace() or load_laplace_state() first")
        return {"A": st["A"].clone(), "G_sum": st["G_sum"].clone(), "sums": st["sums"].clone(),
                "prior_precision": st["info"]["prior_precision"], "head_sha256": st["head_sha256"]}

    def load_laplace_state(self, sd):
        """Install a saved fit (laplace_state_dict()); a fit of another head -- other shapes or other bytes -- is refused."""
        if not (isinstance(sd, dict) and {"A", "G_sum", "sums", "prior_precision", "head_sha256"} <= set(sd)):
            raise native.UvitError("load_laplace_state takes a dict of laplace_state_dict()")
        head = self._head_host()
        if sd["head_sha256"] != self._head_hash(head):
            raise native.UvitError("the Laplace state was fitted on another head (the hash of head.weight / head.bias differs): fit again")
        self.set_laplace(None)
        return self._install(sd["A"], sd["G_sum"], sd["sums"], sd["prior_precision"], head)

    # ---- forward ----
    def _variance_into(self, B):
        """var of self._feat[:B] into self._lap_var[:B]."""
        st = self._lap
        self._lap_buffers_for(B)
        check(lib().uvit_op_lap_variance(ptr(self._feat), ptr(st["UA"]), ptr(st["T"]), ptr(self._lap_var), ptr(self._lap_ws),
                                         self._lap_ws.numel(), B, self.embed_dim, self.num_classes, cur_stream()), "uvit_op_lap_variance")

    def _logits_into(self, B):
        super()._logits_into(B)
        if self._lap is None:
            return
        K = self.num_classes
        self._variance_into(B)
        check(lib().uvit_op_lap_probit(ptr(self._logits), K, ptr(self._lap_var), C.c_double(PROBIT_FACTOR), ptr(self._logits), K,
                                       ptr(self._lap_col), B, K, cur_stream()), "uvit_op_lap_probit")
        self._own_column("lap_var", self._lap_col, B, self._var_slabs)      # the variance of the predicted class

    def predictive_variance(self, images):
        """(B, K) float64 on the device: the diagonal of J (G (x) A + tau I)^-1 J^T at the images' features."""
        if self._lap is None:
            raise native.UvitError("predictive_variance needs fit_laplace() or load_laplace_state() first")
        B = self._features(images)
        self._variance_into(B)
        return self._lap_var[:B].clone()

    # ---- evaluation ----
    def evaluate(self, loader, calibration=False, detection=False, ood_loader=None, variance=True, temperature=None):
        """LinearProbe.evaluate; with a fit, on the probit-scaled logits z~ (loss, accuracy, calibration and the msp / entropy / energy
        columns see them, the post-hoc temperature is applied behind them), detection gains the column `lap_var` (the variance of
        the class the unscaled logits predict) and, with `variance`, the result gains `lap_var_mean`, the mean of that column over
        the evaluation set, from per-batch device slabs read after the last batch.  Without a fit: LinearProbe.evaluate's launches
        and result."""
        return self._evaluate_with_mean("lap_var_mean", variance and self._lap is not None, loader, calibration=calibration,
                                        detection=detection, ood_loader=ood_loader, temperature=temperature)
