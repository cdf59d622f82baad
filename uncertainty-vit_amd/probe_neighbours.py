"""Neighbour bank of the probe: k-NN OOD score and weighted k-NN classifier (csrc/knn.hip).  NeighbourBank is
the score (probe_util.FeatureScore); NeighbourMethods are LinearProbe's public methods for it."""
import ctypes as C
import math

import torch

from . import native
from .native import check, cur_stream, lib, ptr
from .probe_density import MAHA_MAX_K
from .probe_util import FeatureScore, grown, labelled_batches, workspace

KNN_MAX_K, KNN_MAX_N, KNN_MAX_C = 256, 1 << 22, 2048       # csrc/knn.hip: 1 <= k <= 256, 1 <= N <= 2^22, C % 32 == 0, 32 <= C <= 2048
KNN_COLUMNS = ("knn",)                       # the detection column a neighbour bank appends behind the class's and MAHA_COLUMNS
KNN_K, KNN_TEMPERATURE = 20, 0.07            # the weighted k-NN classifier of DINO / iBOT
STATE_KEYS = ("bank", "labels", "sums", "k", "temperature")


def _settings(k, temperature):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= KNN_MAX_K:
        raise native.UvitError(f"k must be a whole number in [1, {KNN_MAX_K}], got {k}")
    T = float(temperature)
    if not 0.0 < T < math.inf:
        raise native.UvitError(f"the k-NN temperature must be positive and finite, got {temperature}")
    return int(k), T


class NeighbourBank(FeatureScore):
    """State: the device bank (n, C) bfloat16 and labels (n) int32, the host sums and `info`."""
    columns, stat_prefix, device_keys = KNN_COLUMNS, "knn", ("bank", "labels")
    fitters = "fit_neighbours() or load_neighbour_state()"

    def check_dims(self):
        K, Cd = self.probe.num_classes, self.probe.embed_dim
        if Cd < 32 or Cd % 32 or Cd > KNN_MAX_C or not 2 <= K <= MAHA_MAX_K:
            raise native.UvitError(f"the k-NN ops take an embed dim that is a multiple of 32 in [32, {KNN_MAX_C}] and 2 .. {MAHA_MAX_K} "
                                   f"classes, got {Cd} and {K}")

    def install(self, bank, labels, sums, k, temperature, own=False):
        """A bank of unit bf16 rows (n, C), their int32 labels (-1: a skipped row) and sums = {rows used, rows skipped} become the
        state in use, on the probe's device (`own`: written by fit() just now, the labels need no look)."""
        k, T = _settings(k, temperature)
        self.check_dims()
        K, Cd = self.probe.num_classes, self.probe.embed_dim
        if not (torch.is_tensor(bank) and torch.is_tensor(labels)) or bank.dtype != torch.bfloat16 or labels.dtype != torch.int32:
            raise native.UvitError("the neighbour state holds a bfloat16 bank and int32 labels")
        if bank.ndim != 2 or bank.shape[1] != Cd or tuple(labels.shape) != (bank.shape[0],) or not 1 <= bank.shape[0] <= KNN_MAX_N:
            raise native.UvitError(f"the neighbour state belongs to another probe: its bank must have shape (n, {Cd}) with 1 <= n <= "
                                   f"{KNN_MAX_N} and one label per row")
        sums = torch.as_tensor(sums, dtype=torch.float64).cpu().contiguous()
        if tuple(sums.shape) != (2,):
            raise native.UvitError("the neighbour state's sums must be {rows used, rows skipped}")
        if not own and (int(labels.max()) >= K or int(labels.min()) < -1):
            raise native.UvitError(f"the neighbour state belongs to another probe: its labels must lie in [-1, {K})")
        n, skipped = int(sums[0]), int(sums[1])
        if n < k:
            raise native.UvitError(f"the neighbour bank holds {n} usable rows (finite features, a label inside [0, K)), fewer than k = {k}")
        dev = self.probe._arena.device
        self.state = {"bank": bank.contiguous().to(dev), "labels": labels.contiguous().to(dev), "sums": sums,
                      "info": {"n": n, "skipped": skipped, "classes": K, "k": k, "temperature": T}}
        self.batch = 0
        self.probe._det_refresh()
        return self.info

    def fit(self, loader, k, temperature):
        k, T = _settings(k, temperature)
        self.check_dims()
        p = self.probe
        K, Cd = p.num_classes, p.embed_dim
        try:
            hint = min(KNN_MAX_N, max(0, len(loader.dataset)))
        except (AttributeError, TypeError):
            hint = 0
        store = sums = None
        n = 0
        for images, labels, B in labelled_batches(p, loader):
            store = grown(store, n, n + B, KNN_MAX_N, f"a neighbour bank holds at most {KNN_MAX_N} rows, the loader holds more",
                          (((None, Cd), torch.bfloat16, 0), ((None,), torch.int32, -1)), images.device, hint)
            bank, lab = store
            if sums is None:
                sums = torch.zeros(2, dtype=torch.float64, device=images.device)
            check(lib().uvit_op_knn_rows(ptr(p._feat), ptr(labels), C.c_void_p(bank.data_ptr() + 2 * n * Cd),
                                         C.c_void_p(lab.data_ptr() + 4 * n), ptr(sums), B, Cd, K, cur_stream()), "uvit_op_knn_rows")
            n += B
        if store is None:
            raise native.UvitError("the neighbour fit needs at least k labelled samples")
        return self.install(bank[:n].clone(), lab[:n].clone(), sums.cpu(), k, T, own=True)       # the one read

    def set_k(self, k, temperature):
        st = self.need("set_neighbours_k")
        k, T = _settings(k, st["info"]["temperature"] if temperature is None else temperature)
        if st["info"]["n"] < k:
            raise native.UvitError(f"the neighbour bank holds {st['info']['n']} usable rows, fewer than k = {k}")
        st["info"].update(k=k, temperature=T)
        self.batch = 0
        return self.info

    def buffers_for(self, B):
        st, p = self.state, self.probe
        k, n, Cd, dev = st["info"]["k"], st["bank"].shape[0], p.embed_dim, p._arena.device
        if st["bank"].device != dev:
            raise native.UvitError("the neighbour bank and the probe are on different devices")
        if B > self.batch:
            self.query = torch.zeros(B, Cd, dtype=torch.bfloat16, device=dev)
            self.valid, self.pred = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
            self.sim = torch.zeros(B, k, dtype=torch.float32, device=dev)
            self.idx = torch.zeros(B, k, dtype=torch.int32, device=dev)
            self.col = torch.zeros(B, dtype=torch.float32, device=dev)
            self.batch = B
        workspace(self, "ws", dev, lib().uvit_op_knn_search_ws_bytes, B, Cd, n, k, 0)

    def into(self, feat, B, labels=None, correct=None):
        """uvit_op_knn_rows, uvit_op_knn_search and uvit_op_knn_scores of feat[:B] on the current stream into self.sim, self.idx
        (B, k), self.col and self.pred."""
        st, p = self.need("the k-NN scores", "need"), self.probe
        p._need_gpu("the k-NN scores run")
        self.buffers_for(B)
        K, Cd, k, n = p.num_classes, p.embed_dim, st["info"]["k"], st["bank"].shape[0]
        s = cur_stream()
        check(lib().uvit_op_knn_rows(ptr(feat), None, ptr(self.query), ptr(self.valid), None, B, Cd, K, s), "uvit_op_knn_rows")
        check(lib().uvit_op_knn_search(ptr(self.query), ptr(self.valid), ptr(st["bank"]), ptr(st["labels"]), ptr(self.sim), ptr(self.idx), k,
                                       ptr(self.ws), self.ws.numel(), B, Cd, n, k, 0, s), "uvit_op_knn_search")
        check(lib().uvit_op_knn_scores(ptr(self.sim), ptr(self.idx), k, ptr(st["labels"]), n, ptr(self.col), ptr(self.pred), None, 0,
                                       ptr(labels), ptr(correct), B, k, K, C.c_double(st["info"]["temperature"]), s), "uvit_op_knn_scores")

    def result(self, feat, B, neighbours):
        self.into(feat, B)
        out = {"knn": self.col[:B].clone(), "pred": self.pred[:B].clone()}
        if neighbours:
            out["sim"], out["idx"] = self.sim[:B].clone(), self.idx[:B].clone()
        return out

    def eval_batch(self, B, labels, ev):
        """Inside evaluate(detection=True): the column of the probe's features into the store (behind the density's, in front of
        _det_rows).  The evaluation set's rows (labels given) are also counted against their labels and kept for the mean."""
        self.into(self.probe._feat, B, labels, ev["correct"] if labels is not None else None)
        self.probe._own_column("knn", self.col, B, ev["slabs"])


class NeighbourMethods:
    """LinearProbe's methods for its NeighbourBank, `self._bank`."""
    _knn = property(lambda self: self._bank.state, doc="the bank's state dict, None when there is none")

    def fit_neighbours(self, loader, k=KNN_K, temperature=KNN_TEMPERATURE):
        """A bank of the training features for nearest-neighbour search: one pass over a labelled loader (items as evaluate()'s) of
        the encoder forward, pool + norm and uvit_op_knn_rows, which appends the batch's unit bf16 rows and int32 labels to a device
        bank (allocated once when the loader's data set has a length, grown geometrically otherwise); the two counters are read once,
        at the end.  Nothing is trained and the head takes no part.  Returns {n (usable rows), skipped (rows with a non-finite
        feature, a zero norm or a label outside [0, K): kept as zero rows that are never a neighbour), classes, k, temperature};
        fewer usable rows than k are refused."""
        return self._bank.fit(loader, k, temperature)

    def set_neighbours(self, state):
        """None forgets the bank (the detection columns are what they were); a dict of neighbour_state_dict() is loaded."""
        if state is not None:
            return self.load_neighbour_state(state)
        self._bank.batch = 0
        self._bank.forget()

    @property
    def neighbours(self):
        """{n, skipped, classes, k, temperature} of the bank in use, None when there is none."""
        return self._bank.info

    def set_neighbours_k(self, k, temperature=None):
        """Another k (and temperature) for the bank in use; the data are not read again."""
        return self._bank.set_k(k, temperature)

    def neighbour_state_dict(self):
        """What a bank is made of, on the host: bank (n, C) bfloat16, labels (n) int32, sums = {rows used, rows skipped}, k and
        temperature.  Not part of state_dict(): neither a parameter nor a buffer."""
        st = self._bank.need("neighbour_state_dict")
        return {"bank": st["bank"].cpu().clone(), "labels": st["labels"].cpu().clone(), "sums": st["sums"].clone(), "k": st["info"]["k"],
                "temperature": st["info"]["temperature"]}

    def load_neighbour_state(self, sd):
        """Install a saved bank (neighbour_state_dict()); one of another embed dim or class count is refused."""
        if not (isinstance(sd, dict) and set(STATE_KEYS) <= set(sd)):
            raise native.UvitError("load_neighbour_state takes a dict of neighbour_state_dict()")
        return self._bank.install(*(sd[k] for k in STATE_KEYS))

    def neighbour_scores(self, images, neighbours=False):
        """{"knn" (B) fp32, "pred" (B) int32} of the images' features against the bank in use, device tensors; with `neighbours`, also
        "sim" (B, k) fp32 and "idx" (B, k) int32, the k nearest bank rows by (similarity descending, index ascending).  knn = 2 - 2 s_k,
        the squared distance between the unit vectors to the k-th nearest bank row (larger = more out of distribution); pred = the
        class with the largest vote sum_j exp((s_j - s_1) / T) over the k neighbours.  A row with a non-finite feature: NaN, -1."""
        self._bank.need("neighbour_scores")
        B = self._features(images)
        return self._bank.result(self._feat, B, neighbours)

    def neighbour_batch(self, feat, neighbours=False):
        """neighbour_scores() of caller-supplied GPU features (B, C) fp32; nothing synchronises with the host."""
        return self._bank.result(feat, self._check_feat(feat), neighbours)
