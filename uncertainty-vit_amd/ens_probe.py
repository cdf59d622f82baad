"""Ensemble probe on the frozen encoder: M linear heads behind the pooled features of the linear probe, trained side by side and
combined on the device -- the deep ensemble the reference evaluates with `--ensembles` (engine_for_finetuning.ensembles_evaluate,
:225-343: separately trained checkpoints, each run over the evaluation set, then the metrics of the mean of their logits), DESIGN.md
section 9.5.

    pooled features f (linear_probe.py) -> lin = f . W^T + bias, W (M K, C): member m owns rows m K .. (m + 1) K - 1
    z = mean_m lin_m ("logits", the reference's)   or   z = log mean_m softmax(lin_m) ("probs")

The encoder is frozen and is nearly all of a probe step, so the members share one encoder forward per batch; the M heads are the rows
of ONE matrix in one arena, so the forward is one uvit_op_probe_logits call and the head gradient one uvit_op_probe_head_grad call.
The members' losses, the optional online-bagging weights (Oza & Russell: a Poisson(1) weight per member and sample presentation,
counter-based, nothing stored), the per-member gradient clip and the combination with its entropy split are the kernels of
csrc/ens.hip.  Each member receives exactly the gradient it would receive alone, and the clip is per member: without bagging member m
trains as a LinearProbe started from its initial values would.
"""
import math

import torch
import torch.nn as nn

from .het_probe import _hash32
from .linear_probe import LinearProbe, _timm_trunc_normal_
from .modeling_cyclical import _Holder
from .native import check, cur_stream, f32, lib, ptr

__all__ = ["EnsembleProbe"]

MAX_MEMBERS = 16             # csrc/ens.hip: 1 <= M <= 16
COMBINE_MODES = {"logits": 0, "probs": 1}
UNC_KEYS = ("ens_total", "ens_aleatoric", "ens_mi", "ens_var", "ens_disagreement")      # the columns of uvit_op_ens_combine's unc


class EnsembleProbe(LinearProbe):
    """state_dict() holds `heads.{m}.weight` (K, C) and `heads.{m}.bias` (K,) for m = 0 .. M-1; member_state_dict(m) gives member m
    under a LinearProbe's keys.  `combine`: "logits" (the mean of the members' logits, the reference's) or "probs" (the logarithm of the
    mean of their softmaxes).  `bagging`: train member m on Poisson(1)-weighted samples under `seed` (off by default: an addition to
    the reference).  `member_norms` (M,) holds the members' gradient norms of the last train_step, on the device."""

    def __init__(self, encoder, num_classes, members=5, smoothing=0.1, init_scale=0.001, combine="logits", bagging=False, seed=0):
        M = int(members)
        if not 1 <= M <= MAX_MEMBERS:
            raise ValueError(f"members must be in [1, {MAX_MEMBERS}], got {members}")
        if combine not in COMBINE_MODES:
            raise ValueError(f"combine must be one of {sorted(COMBINE_MODES)}, got {combine!r}")
        self.members, self.combine, self.bagging, self.seed = M, combine, bool(bagging), int(seed) & 0xFFFFFFFF
        super().__init__(encoder, num_classes, smoothing=smoothing, init_scale=init_scale)

    # ---- arena plumbing ----
    @property
    def _OPT_KEYS(self):
        return [f"heads.{m}.{n}" for n in ("weight", "bias") for m in range(self.members)]

    def _views(self):
        """(parameter, lo, hi, shape) in arena order: [W_0 | ... | W_{M-1} | b_0 | ... | b_{M-1} | pad to 4]."""
        K, Cd, M = self.num_classes, self.embed_dim, self.members
        w0 = M * K * Cd
        heads = [getattr(self.heads, str(m)) for m in range(M)]
        return tuple((h.weight, m * K * Cd, (m + 1) * K * Cd, (K, Cd)) for m, h in enumerate(heads)) + \
            tuple((h.bias, w0 + m * K, w0 + (m + 1) * K, (K,)) for m, h in enumerate(heads))

    def _setup_head(self, init_scale):
        K, Cd, M = self.num_classes, self.embed_dim, self.members
        self._rows = M * K                       # the M heads as one (M K, C) matrix and one bias vector
        self._n_decay = self._rows * Cd          # the weights decay, the biases do not
        n = (self._n_decay + self._rows + 3) // 4 * 4
        dev = self.encoder._arena.device
        self._arena, self._grad_arena, self.exp_avg, self.exp_avg_sq = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(4))
        self.member_norms = torch.zeros(M, dtype=torch.float32, device=dev)
        self.step_count = 0
        self.heads = _Holder()
        for m in range(M):
            h = _Holder()
            h.register_parameter("weight", nn.Parameter(self._arena[m * K * Cd:(m + 1) * K * Cd].view(K, Cd)))
            h.register_parameter("bias", nn.Parameter(self._arena[self._n_decay + m * K:self._n_decay + (m + 1) * K]))
            self.heads.add_module(str(m), h)
        self._rebind()
        # every member as LinearProbe initialises its head (modeling_finetune.py:439-441), drawn on the host in member order under
        # the caller's seed; the biases stay 0
        with torch.no_grad():
            for m in range(M):
                getattr(self.heads, str(m)).weight.copy_(_timm_trunc_normal_(torch.empty(K, Cd), std=0.02).mul_(init_scale))
        self._eval = None

    def _apply(self, fn, recurse=True):
        self.member_norms = fn(self.member_norms)
        return super()._apply(fn, recurse)

    def _vim_head(self):
        """combine="logits": the mean of the members' heads, whose logits are the mean of theirs; "probs" is not affine."""
        if self.combine != "logits":
            self._vim_not_affine('the ensemble with combine="probs" reports the logarithm of a mean of softmaxes')
        heads = [getattr(self.heads, str(m)) for m in range(self.members)]
        return (torch.stack([h.weight.detach().to("cpu", torch.float64) for h in heads]).mean(0),
                torch.stack([h.bias.detach().to("cpu", torch.float64) for h in heads]).mean(0))

    def _head_buffers_for(self, B):
        M, dev = self.members, self._arena.device
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
        self._lin, self._dlin, self._bag, self._member_rows = z(B, self._rows), z(B, self._rows), z(B, M), z(B, M)
        self._member_loss = z(M + 1)             # the members' losses of the last train_step, then their mean
        self._unc = z(B, 5, dt=torch.float64)

    # ---- forward ----
    def _lin_into(self, B):
        check(lib().uvit_op_probe_logits(ptr(self._feat), ptr(self._arena), self._bias_ptr(self._arena), ptr(self._lin), B, self._rows,
                                         self.embed_dim, cur_stream()), "uvit_op_probe_logits")

    def _combine_into(self, B, unc=None):
        check(lib().uvit_op_ens_combine(ptr(self._lin), COMBINE_MODES[self.combine], ptr(self._logits), ptr(unc), B, self.members,
                                        self.num_classes, cur_stream()), "uvit_op_ens_combine")

    def _labels(self, labels, B):
        labels = super()._labels(labels, B)
        if self._eval is not None:
            self._eval["labels"] = labels
        return labels

    def _logits_into(self, B):
        """The members' logits, then the combination z into self._logits.  Inside evaluate(members=, uncertainty=) the members'
        criterion and the uncertainty columns of the batch go to device slabs that are read after the last batch."""
        self._lin_into(B)
        ev, det = self._eval, self._det is not None
        slab = None
        if det or (ev is not None and ev["unc"] is not None):
            slab = torch.zeros(B, 5, dtype=torch.float64, device=self._arena.device)
            if ev is not None and ev["unc"] is not None and not self._in_ood:
                ev["unc"].append(slab)
        self._combine_into(B, slab)
        if det:      # evaluate(detection=True): the five columns of the batch go to the set-level store
            for col, name in enumerate(UNC_KEYS):
                self._own_column(name, slab[:, col], B, None)
        if ev is not None and ev["losses"] is not None and ev.get("labels") is not None:
            M, dev = self.members, self._arena.device
            if ev["counters"] is None:
                ev["counters"] = torch.zeros(M, 2, dtype=torch.int32, device=dev)
            out = torch.zeros(M + 1, dtype=torch.float32, device=dev)
            check(lib().uvit_op_ens_ce(ptr(self._lin), ptr(ev["labels"]), None, f32(0.0), None, ptr(self._member_rows), ptr(out),
                                       ptr(ev["counters"]), B, M, self.num_classes, cur_stream()), "uvit_op_ens_ce")
            ev["losses"].append((out, B))
            ev["labels"] = None

    def member_logits(self, images):
        """(B, M, K) fp32: every member's logits."""
        B = self._features(images)
        self._lin_into(B)
        return self._lin[:B].view(B, self.members, self.num_classes).clone()

    def uncertainty(self, images):
        """(B, 5) float64 per sample: the entropy of the mean of the members' softmaxes, the mean of the members' entropies, their
        difference (the mutual information between prediction and member, clamped at 0), the variance over the members of the
        probability of the ensemble's predicted class, and the fraction of members whose prediction differs from the ensemble's."""
        B = self._features(images)
        self._lin_into(B)
        self._combine_into(B, self._unc)
        return self._unc[:B].clone()

    # ---- training ----
    def step_seed(self, step):
        """The bagging seed of training step `step` (0-based): fresh weights for every presentation of a sample."""
        return _hash32(self.seed ^ ((step * 0x85EBCA6B + 1) & 0xFFFFFFFF))

    def enable_mix(self, mixer):
        """Not built: the ensemble's loss is uvit_op_ens_ce with its bagging weights, and no soft-target form of it exists."""
        if mixer is not None:
            raise NotImplementedError("mixup / cutmix / random erasing under the ensemble is not built: its loss is uvit_op_ens_ce")

    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        """One step on the M heads, as LinearProbe.train_step: one logits call, the members' cross-entropies (weighted by the bagging
        weights of step_seed(step_count) when bagging), one head-gradient call, the per-member clip (max_norm) and one AdamW over
        the arena.  Returns (mean of the members' losses, norm of the whole gradient arena after the clip) as device scalars; the
        members' losses stay in self._member_loss[:M], their gradient norms before the clip in self.member_norms.  With an augmenter
        (enable_randaug) the batch goes through RandAugment first; a mixer is refused (enable_mix)."""
        B = self._features(self._train_images(images))
        labels = self._labels(labels, B)
        M, K, Cd, L, s = self.members, self.num_classes, self.embed_dim, lib(), cur_stream()
        self._lin_into(B)
        if self.bagging:
            check(L.uvit_op_ens_bag_weights(ptr(self._bag), B, M, self.step_seed(self.step_count), s), "uvit_op_ens_bag_weights")
        check(L.uvit_op_ens_ce(ptr(self._lin), ptr(labels), ptr(self._bag if self.bagging else None), f32(self.smoothing), ptr(self._dlin),
                               ptr(self._member_rows), ptr(self._member_loss), None, B, M, K, s), "uvit_op_ens_ce")
        check(L.uvit_op_probe_head_grad(ptr(self._dlin), ptr(self._feat), ptr(self._grad_arena), self._bias_ptr(self._grad_arena), B, self._rows,
                                        Cd, s), "uvit_op_probe_head_grad")
        check(L.uvit_op_ens_clip(ptr(self._grad_arena), ptr(self.member_norms), M, K, Cd,
                                 f32(max_norm if max_norm is not None and max_norm > 0 else 0.0), s), "uvit_op_ens_clip")
        _, gnorm = self._clip_and_update(lr, weight_decay, None)
        return self._member_loss[M], gnorm

    # ---- evaluation ----
    DETECT_COLUMNS = LinearProbe.DETECT_COLUMNS + UNC_KEYS

    def evaluate(self, loader, calibration=False, members=False, uncertainty=False, detection=False, ood_loader=None, temperature=None):
        """LinearProbe.evaluate on z.  `members`: the result gains the lists `member_loss`, `member_acc1`, `member_acc5` (plain
        cross-entropy and accuracies in percent of every member, one uvit_op_ens_ce call per batch) and `member_correct1`,
        `member_correct5`.  `uncertainty`: the means over the set of the five columns of uncertainty() as `ens_total`, `ens_aleatoric`,
        `ens_mi`, `ens_var`, `ens_disagreement`, over the rows without a NaN; `ens_nan_rows` counts the others.  Everything comes
        from per-batch device slabs that are read once, after the last batch.  `detection`, `ood_loader`: as LinearProbe.evaluate on
        z, with the five columns of uncertainty() beside the three of the logits, whatever `uncertainty` says.  `temperature`: as
        LinearProbe.evaluate, on the combined z; the members' own lines and the five ens_* columns come from the members' logits
        before the combination and are not scaled."""
        self._eval = {"losses": [] if members else None, "unc": [] if uncertainty else None, "counters": None, "labels": None}
        try:
            stats = super().evaluate(loader, calibration=calibration, detection=detection, ood_loader=ood_loader, temperature=temperature)
            ev, M, n = self._eval, self.members, stats["n"]
            if members:
                nan = [float("nan")] * M
                stats.update(member_loss=nan, member_acc1=list(nan), member_acc5=list(nan))
                if n:
                    host = torch.stack([t for t, _ in ev["losses"]]).cpu().double()          # (batches, M + 1)
                    sizes = torch.tensor([b for _, b in ev["losses"]], dtype=torch.float64)
                    cnt = ev["counters"].cpu().tolist()
                    stats["member_loss"] = ((host[:, :M] * sizes[:, None]).sum(0) / n).tolist()
                    stats["member_correct1"], stats["member_correct5"] = [c[0] for c in cnt], [c[1] for c in cnt]
                    stats["member_acc1"], stats["member_acc5"] = [100.0 * c[0] / n for c in cnt], [100.0 * c[1] / n for c in cnt]
            if uncertainty:
                rows = torch.cat(ev["unc"]).cpu().tolist() if ev["unc"] else []
                good = [r for r in rows if not any(math.isnan(v) for v in r)]
                stats["ens_nan_rows"] = len(rows) - len(good)
                for col, key in enumerate(UNC_KEYS):
                    stats[key] = math.fsum(r[col] for r in good) / len(good) if good else float("nan")
        finally:
            self._eval = None
        return stats

    # ---- members in and out ----
    def _member(self, m):
        if not 0 <= int(m) < self.members:
            raise IndexError(f"member {m} outside [0, {self.members})")
        return getattr(self.heads, str(int(m)))

    def member_state_dict(self, m):
        """Member m under the keys of a LinearProbe: {"head.weight" (K, C), "head.bias" (K,)}, on the host."""
        h = self._member(m)
        return {"head.weight": h.weight.detach().cpu().clone(), "head.bias": h.bias.detach().cpu().clone()}

    def load_member(self, m, sd):
        """Member m from a LinearProbe's state dict."""
        h = self._member(m)
        K, Cd = self.num_classes, self.embed_dim
        w, b = sd["head.weight"], sd["head.bias"]
        if tuple(w.shape) != (K, Cd) or tuple(b.shape) != (K,):
            raise ValueError(f"member {m}: head.weight {tuple(w.shape)} / head.bias {tuple(b.shape)} are not ({K}, {Cd}) / ({K},)")
        with torch.no_grad():
            h.weight.copy_(w)
            h.bias.copy_(b)

    @classmethod
    def from_heads(cls, encoder, heads, **kw):
        """An ensemble of separately trained linear-probe heads (the reference's workflow): `heads` is a list of LinearProbe state
        dicts; the member count is its length."""
        heads = list(heads)
        if not heads:
            raise ValueError("from_heads needs at least one head")
        probe = cls(encoder, heads[0]["head.weight"].shape[0], members=len(heads), **kw)
        for m, sd in enumerate(heads):
            probe.load_member(m, sd)
        return probe
