"""ViM of the probe: the residual of the feature off the training features' principal space, matched to the logits (csrc/vim.hip,
DESIGN.md section 9.13).  VimScore is the score (probe_util.FeatureScore); VimMethods are LinearProbe's public methods for it."""
import ctypes as C
import math

import torch

from . import native
from .native import check, cur_stream, lib, ptr
from .probe_density import MAHA_MAX_C, MAHA_MAX_K
from .probe_util import FeatureScore, image_batches, workspace

VIM_COLUMNS = ("vim", "residual")            # the detection columns a ViM fit appends behind the class's, MAHA_COLUMNS and KNN_COLUMNS
STATE_KEYS = ("R", "origin", "weight", "bias", "alpha", "dim", "eigenvalues", "sums")


def vim_default_dim(Cd):
    """The paper's principal dimension D: 1000 for C >= 2048, 512 for C >= 768, otherwise C // 2."""
    return 1000 if Cd >= 2048 else 512 if Cd >= 768 else Cd // 2


class VimScore(FeatureScore):
    """State: the host float64 R (Cn, C), origin (C), weight (K, C), bias (K), eigenvalues (C, ascending) and sums = {sum of max z, sum
    of residual, rows used, rows skipped}, the device float64 A = [R ; weight] and a = [-R origin ; bias], and `info`."""
    columns, stat_prefix, device_keys = VIM_COLUMNS, "vim", ("A", "a")
    fitters = "fit_vim() or load_vim_state()"

    def check_dims(self):
        K, Cd = self.probe.num_classes, self.probe.embed_dim
        if Cd < 4 or Cd % 4 or Cd > MAHA_MAX_C or not 2 <= K <= MAHA_MAX_K:
            raise native.UvitError(f"the ViM op takes an embed dim that is a multiple of 4 in [4, {MAHA_MAX_C}] and 2 .. {MAHA_MAX_K} classes, "
                                   f"got {Cd} and {K}")
        return K, Cd

    def dim(self, dim):
        """The principal dimension D as an int; it lies in [1, C - 1]."""
        Cd = self.probe.embed_dim
        if isinstance(dim, bool) or int(dim) != dim or not 1 <= int(dim) <= Cd - 1:
            raise native.UvitError(f"dim must be a whole number in [1, {Cd - 1}], got {dim}")
        return int(dim)

    def head(self, head):
        """(W (K, C), b (K)) float64 on the host: the caller's, or the probe's own affine head as it stands."""
        K, Cd = self.check_dims()
        W, b = self.probe._vim_head() if head is None else head
        W, b = (torch.as_tensor(t).detach().to("cpu", torch.float64).contiguous() for t in (W, b))
        if tuple(W.shape) != (K, Cd) or tuple(b.shape) != (K,) or not bool(torch.isfinite(W).all() and torch.isfinite(b).all()):
            raise native.UvitError(f"the head of a ViM fit is a finite weight ({K}, {Cd}) and bias ({K},)")
        return W, b

    def candidate(self, R, origin, weight, bias, dim, eigenvalues):
        """A state without alpha and sums from its host parts: shapes checked, A and a stacked and uploaded."""
        K, Cd = self.check_dims()
        D, F64 = self.dim(dim), torch.float64
        R, origin, weight, bias, eigenvalues = (torch.as_tensor(t, dtype=F64).cpu().contiguous() for t in (R, origin, weight, bias, eigenvalues))
        if (tuple(R.shape), tuple(origin.shape), tuple(weight.shape), tuple(bias.shape), tuple(eigenvalues.shape)) != \
                ((Cd - D, Cd), (Cd,), (K, Cd), (K,), (Cd,)):
            raise native.UvitError(f"the ViM state belongs to another probe: R, origin, weight, bias and eigenvalues must have shapes "
                                   f"({Cd - D}, {Cd}), ({Cd},), ({K}, {Cd}), ({K},) and ({Cd},)")
        A, a = torch.cat([R, weight]), torch.cat([-(R @ origin), bias])
        if not bool(torch.isfinite(A).all() and torch.isfinite(a).all()):
            raise native.UvitError("the ViM fit failed: the stacked matrix is not finite (non-finite features or head?)")
        dev = self.probe._arena.device
        total = float(eigenvalues.sum())
        return {"R": R, "origin": origin, "weight": weight, "bias": bias, "eigenvalues": eigenvalues, "A": A.contiguous().to(dev),
                "a": a.contiguous().to(dev), "dim": D, "explained": float(eigenvalues[Cd - D:].sum()) / total if total > 0 else float("nan")}

    def finish(self, st, alpha, sums):
        """`st` of candidate() with its alpha and sums becomes the state in use."""
        sums = torch.as_tensor(sums, dtype=torch.float64).cpu().contiguous()
        if tuple(sums.shape) != (4,):
            raise native.UvitError("the ViM state's sums must be {sum of max z, sum of residual, rows used, rows skipped}")
        alpha = float(alpha)
        if not math.isfinite(alpha):
            raise native.UvitError(f"the ViM alpha must be finite, got {alpha}")
        st.update(alpha=alpha, sums=sums,
                  info={"n": int(sums[2]), "skipped": int(sums[3]), "classes": self.probe.num_classes, "dim": st["dim"], "alpha": alpha,
                        "explained": st["explained"]})
        self.state = st
        self.probe._det_refresh()
        return self.info

    def install(self, R, origin, weight, bias, alpha, dim, eigenvalues, sums):
        return self.finish(self.candidate(R, origin, weight, bias, dim, eigenvalues), alpha, sums)

    def moments(self, loader, moments):
        """(S (C, C), t (C), n) float64 on the host: pass 1 over the loader, or the sums of a density fitted on the same data."""
        K, Cd = self.check_dims()
        if moments is None:
            got = self.probe._density.accumulate(loader)
            if got is None:
                raise native.UvitError("the ViM fit needs at least two labelled samples")
            S, _, t, _, sums = got
        else:
            if not (isinstance(moments, dict) and {"S", "total_sum", "sums"} <= set(moments)):
                raise native.UvitError("moments takes a dict of density_state_dict()")
            S, t, sums = (torch.as_tensor(moments[k], dtype=torch.float64).cpu() for k in ("S", "total_sum", "sums"))
            if (tuple(S.shape), tuple(t.shape), tuple(sums.shape)) != ((Cd, Cd), (Cd,), (2,)):
                raise native.UvitError(f"the moments belong to another probe: S, total_sum and sums must have shapes ({Cd}, {Cd}), ({Cd},) and (2,)")
        n = float(sums[0])
        if not n >= 2:
            raise native.UvitError("the ViM fit needs at least two usable rows (finite features, a label inside [0, K))")
        return S, t, n

    def fit(self, loader, dim, head, moments):
        K, Cd = self.check_dims()
        D = self.dim(vim_default_dim(Cd) if dim is None else dim)
        W, b = self.head(head)
        self.probe._need_gpu("the ViM fit runs")
        S, t, n = self.moments(loader, moments)
        o = -(torch.linalg.pinv(W) @ b)
        M = (S - torch.outer(o, t) - torch.outer(t, o) + n * torch.outer(o, o)) / n
        M = 0.5 * (M + M.T)
        if not bool(torch.isfinite(M).all()):
            raise native.UvitError("the ViM fit failed: the second moment of the features is not finite")
        lam, V = torch.linalg.eigh(M)                                   # ascending: the first Cn columns span the null space in use
        st = self.candidate(V[:, :Cd - D].T.contiguous(), o, W, b, D, lam)
        sums = None
        for images, B in image_batches(self.probe, loader):             # pass 2: the matching constant over the same rows
            if sums is None:
                sums = torch.zeros(4, dtype=torch.float64, device=images.device)
            self.into(self.probe._feat, B, st=st, alpha=0.0, sums=sums)
        if sums is None:
            raise native.UvitError("the ViM fit needs at least two labelled samples")
        host = sums.cpu()                                               # the one read
        if not (float(host[1]) > 0.0 and math.isfinite(float(host[0]))):
            raise native.UvitError("the ViM fit failed: the fit set's residuals do not have a positive sum (dim too large for these features?)")
        return self.finish(st, float(host[0]) / float(host[1]), host)

    def buffers_for(self, B, st):
        p = self.probe
        dev = p._arena.device
        if st["A"].device != dev:
            raise native.UvitError("the ViM state and the probe are on different devices")
        if B > self.batch:
            self.col, self.rcol = (torch.zeros(B, dtype=torch.float32, device=dev) for _ in range(2))
            self.pred = torch.zeros(B, dtype=torch.int32, device=dev)
            self.batch = B
        workspace(self, "ws", dev, lib().uvit_op_vim_scores_ws_bytes, B, p.embed_dim, p.embed_dim - st["dim"], p.num_classes)

    def into(self, feat, B, labels=None, correct=None, st=None, alpha=None, sums=None):
        """uvit_op_vim_scores of feat[:B] on the current stream into self.col, self.rcol and self.pred (`st`, `alpha`, `sums`: the
        fit's second pass, on a state that is not yet in use)."""
        p = self.probe
        if st is None:
            st = self.need("the ViM scores", "need")
        p._need_gpu("the ViM scores run")
        self.buffers_for(B, st)
        Cd = p.embed_dim
        check(lib().uvit_op_vim_scores(ptr(feat), ptr(st["A"]), ptr(st["a"]), C.c_double(st["alpha"] if alpha is None else alpha),
                                       ptr(self.col), ptr(self.rcol), ptr(self.pred), ptr(labels), ptr(correct), ptr(sums), ptr(self.ws),
                                       self.ws.numel(), B, Cd, Cd - st["dim"], p.num_classes, cur_stream()), "uvit_op_vim_scores")

    def result(self, feat, B):
        self.into(feat, B)
        return {"vim": self.col[:B].clone(), "residual": self.rcol[:B].clone(), "pred": self.pred[:B].clone()}

    def eval_batch(self, B, labels, ev):
        """Inside evaluate(detection=True): the two columns of the probe's features into the store (behind the bank's, in front of
        _det_rows).  The evaluation set's rows (labels given) are also counted against their labels and kept for the mean."""
        self.into(self.probe._feat, B, labels, ev["correct"] if labels is not None else None)
        self.probe._own_column("vim", self.col, B, ev["slabs"])
        self.probe._own_column("residual", self.rcol, B, None)


class VimMethods:
    """LinearProbe's methods for its VimScore, `self._vim_score`."""
    _vim = property(lambda self: self._vim_score.state, doc="the ViM state dict, None when there is none")

    def _vim_head(self):
        """(W (K, C), b (K)) of the affine head whose logits the probe reports; a head that is not affine in the feature raises."""
        return self.head.weight, self.head.bias

    def _vim_not_affine(self, what):
        raise native.UvitError(f"{what}: its logits are not affine in the feature, so ViM has no head to take the origin and the logits "
                               f"from; pass one, head=(W, b)")

    def fit_vim(self, loader, dim=None, head=None, moments=None):
        """ViM (virtual-logit matching, Wang et al. 2022) on the probe's features.  The loader (labelled, items as evaluate()'s) is
        walked twice.  Pass 1: the encoder forward, pool + norm and uvit_op_maha_accumulate into device accumulators, one read of
        S = sum f f^T, t = sum f and n; skipped when `moments`, a dict of density_state_dict() fitted on the same data, is given.  The
        host then takes a float64 snapshot (W, b) of the head (`head`, default: the probe's own), the origin o = -pinv(W) b, the
        second moment of f - o, its eigenvectors (torch.linalg.eigh on the CPU) and uploads A = [R ; W] and a = [-R o ; b], R the
        eigenvectors of the C - dim smallest eigenvalues (`dim` defaults to 1000 for C >= 2048, 512 for C >= 768, else C // 2).  Pass 2:
        the forward again and uvit_op_vim_scores with alpha = 0, whose `sums` give alpha = sum max z / sum residual in one read.
        Returns {n, skipped (rows of pass 2 with a non-finite feature), classes, dim, alpha, explained (the share of the trace of
        the second moment in the dim kept eigenvalues)}.  A fit set without a positive residual sum is refused.  The head is a
        snapshot: training it afterwards leaves the state as it is (evaluate's vim_acc1 then reads as a staleness check)."""
        return self._vim_score.fit(loader, dim, head, moments)

    def set_vim(self, state):
        """None forgets the ViM fit (the detection columns are what they were); a dict of vim_state_dict() is loaded."""
        if state is not None:
            return self.load_vim_state(state)
        self._vim_score.forget()

    @property
    def vim(self):
        """{n, skipped, classes, dim, alpha, explained} of the ViM fit in use, None when there is none."""
        return self._vim_score.info

    def vim_state_dict(self):
        """What a ViM fit is made of, on the host in float64: R (C - dim, C), origin (C), weight (K, C), bias (K), alpha, dim,
        eigenvalues (C, ascending) and sums = {sum of max z, sum of residual, rows used, rows skipped}.  Not part of state_dict():
        neither a parameter nor a buffer."""
        st = self._vim_score.need("vim_state_dict")
        return {**{k: st[k].clone() for k in ("R", "origin", "weight", "bias", "eigenvalues", "sums")}, "alpha": st["alpha"], "dim": st["dim"]}

    def load_vim_state(self, sd):
        """Install a saved ViM fit (vim_state_dict()); one of another embed dim or class count is refused."""
        if not (isinstance(sd, dict) and set(STATE_KEYS) <= set(sd)):
            raise native.UvitError("load_vim_state takes a dict of vim_state_dict()")
        return self._vim_score.install(*(sd[k] for k in STATE_KEYS))

    def vim_scores(self, images):
        """{"vim", "residual" (B) fp32, "pred" (B) int32} of the images' features against the ViM fit in use, device tensors.
        residual = |R (f - o)|, the length of the feature's part outside the principal space; vim = alpha residual - logsumexp(z) with
        z the snapshot head's logits; pred = arg max z; larger = more out of distribution.  A row with a non-finite feature: NaN,
        NaN, -1."""
        self._vim_score.need("vim_scores")
        B = self._features(images)
        return self._vim_score.result(self._feat, B)

    def vim_batch(self, feat):
        """vim_scores() of caller-supplied GPU features (B, C) fp32; nothing synchronises with the host."""
        self._vim_score.need("vim_batch")
        return self._vim_score.result(feat, self._check_feat(feat))
