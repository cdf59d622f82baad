"""Host: the tables behind run_linear_probe.main -- report() on hand-made stats for every head with all the families it admits, in
the --eval and the epoch form, against lines and log keys written out here; the refusal of every pair of heads; and the library
defaults that the command line no longer restates, against the values its usage text documents."""
import inspect
from types import SimpleNamespace

import pytest
import torch

import run_linear_probe as rlp

H = 0.5
ROW = {"AUROC": H, "AUPR": H, "FPR95": H, "AURC": H}
STATS = {
    "loss": H, "acc1": 50.0, "acc5": 75.0, "n": 8, "ECE": H, "TACE": H, "NLL": H, "AUROC": H, "temperature": 2.0,
    "set_calibration": {**{k: H for k in ("ECE", "MCE", "OE", "NLL", "Brier", "SCE", "ACE", "TACE", "AUROC")}, "n": 8, "auroc_classes": 3,
                        "reliability": [[1.0, H, H]]},
    "detection": {"columns": ["msp"], "misclassification": {"msp": ROW}, "ood": {"msp": {k: H for k in ("AUROC", "AUPR", "FPR95")}}},
    "conformal": {0.1: {"coverage": H, "size": 2.0, "empty": 0.0, "singleton": H, "sscv": H, "worst_class": H}},
    "lap_var_mean": H, "maha_acc1": 50.0, "maha_mean": H, "knn_acc1": 50.0, "knn_mean": H, "vim_acc1": 50.0, "vim_mean": H,
    "gp_var_mean": H, "het_var_mean": H, "dist_var_mean": H, "dist_trace_mean": H, "layer_weights": [0.25, 0.75],
    "member_acc1": [50.0, 25.0], "member_acc5": [75.0, 75.0], "member_loss": [H, H],
    "ens_total": H, "ens_aleatoric": H, "ens_mi": H, "ens_var": H, "ens_disagreement": H,
    "mcd_total": H, "mcd_aleatoric": H, "mcd_mi": H, "mcd_var": H, "mcd_disagreement": H, "det_acc1": 50.0, "mcd_passes": 4, "mcd_layers": 1,
}
FITS = {
    "calibration": True, "set_calibration": {}, "detection": {"detection": True},
    "temperature": {"T": 2.0, "nll_before": 1.0, "nll_after": H, "n": 8, "iterations": 3, "status": 0},
    "laplace": {"prior_precision": 1.0, "source": "given", "on_grid_edge": False, "log_marglik": -1.0, "nll": 4.0, "n": 8},
    "maha": {"n": 8, "skipped": 0, "classes": 3, "empty_classes": 0, "shrinkage": 0.001, "logdet": H, "logdet0": H},
    "knn": {"n": 8, "skipped": 0, "classes": 3, "k": 2, "temperature": 0.07},
    "vim": {"n": 8, "skipped": 0, "dim": 4, "alpha": H, "explained": H},
    "conformal": {"score": "aps", "alpha": [0.1], "qhat": [H], "n": 8},
}
DIMS = SimpleNamespace(depth=2, attn_drop_rate=0.1, embed_dim=16)

FRONT = {
    "temperature": ["* Temperature 2.00000 NLL 1.00000 -> 0.50000 on 8 calibration images (3 passes, converged)"],
    "laplace": ["* Laplace prior precision 1 (given) log-marglik -1.00000 NLL 0.50000 on 8 images", "* Laplace variance mean 0.500000"],
    "maha": ["* Mahalanobis fit on 8 images (0 skipped), 3 classes (0 empty), shrinkage 0.001, log-det 0.50000 background 0.50000",
             "* Mahalanobis Acc@1 50.000 mean 0.50000"],
    "knn": ["* kNN bank of 8 images (0 skipped), 3 classes, k 2, temperature 0.07", "* kNN Acc@1 50.000 mean 0.50000"],
    "vim": ["* ViM fit on 8 images (0 skipped), dim 4 of 16, alpha 0.50000, explained 0.50000", "* ViM Acc@1 50.000 mean 0.50000"],
}
HEAD_LINES = {
    "gp": ["* GP variance mean 0.500000"],
    "het": ["* Het variance mean 0.500000"],
    "ens": ["* Member 0 Acc@1 50.000 Acc@5 75.000 loss 0.500", "* Member 1 Acc@1 25.000 Acc@5 75.000 loss 0.500",
            "* Ens entropy 0.50000 expected 0.50000 MI 0.50000 variance 0.500000 disagreement 0.50000"],
    "lap": [],
    "mcd": ["* MC-dropout passes 4 layers 1 of 2 rate 0.1 entropy 0.50000 expected 0.50000 MI 0.50000 variance 0.500000 disagreement 0.50000",
            "* Deterministic Acc@1 50.000"],
    "lw": ["* Layer weights 0.2500 0.7500 (argmax: block 1)"],
    "dist": ["* Dist variance mean 0.500000 trace mean 0.500000"],
    "linear": [],
}
BEHIND = {
    "calibration": ["* ECE 0.50000 TACE 0.50000 NLL 0.50000 AUROC 0.50000"],
    "set_calibration": ["* Set ECE 0.50000 MCE 0.50000 OE 0.50000 NLL 0.50000 Brier 0.50000 SCE 0.50000 ACE 0.50000 TACE 0.50000 AUROC 0.50000 "
                        "on 8 images (3 classes with an AUROC)"],
    "detection": ["* Detect misclassification msp AUROC 0.50000 AUPR 0.50000 FPR95 0.50000 AURC 0.50000",
                  "* Detect OOD msp AUROC 0.50000 AUPR 0.50000 FPR95 0.50000"],
    "conformal": ["* Conformal aps alpha 0.1 qhat 0.50000 coverage 0.50000 size 2.000 empty 0.00000 singleton 0.50000 SSCV 0.50000 worst-class 0.50000 "
                  "on 8 calibration images"],
}
HEAD_KEYS = {
    "gp": ["test_gp_var_mean"], "het": ["test_het_var_mean"], "dist": ["test_dist_var_mean", "test_dist_trace_mean"], "lap": [], "linear": [],
    "ens": ["test_member0_acc1", "test_member1_acc1", "test_ens_total", "test_ens_aleatoric", "test_ens_mi", "test_ens_var", "test_ens_disagreement"],
    "mcd": ["test_mcd_total", "test_mcd_aleatoric", "test_mcd_mi", "test_mcd_var", "test_mcd_disagreement", "test_mcd_det_acc1", "test_mcd_passes"],
    "lw": ["test_layer_weights"],
}
LOG_KEYS = {
    "calibration": ["test_ECE", "test_TACE", "test_NLL", "test_AUROC"],
    "set_calibration": ["test_set_ECE", "test_set_MCE", "test_set_OE", "test_set_NLL", "test_set_Brier", "test_set_SCE", "test_set_ACE", "test_set_TACE",
                        "test_set_AUROC", "test_set_reliability"],
    "detection": ["test_mis_msp_AUROC", "test_mis_msp_AUPR", "test_mis_msp_FPR95", "test_mis_msp_AURC", "test_ood_msp_AUROC", "test_ood_msp_AUPR",
                  "test_ood_msp_FPR95"],
    "temperature": ["test_ts_temperature", "test_ts_nll_before", "test_ts_nll_after", "test_ts_n", "test_ts_iterations", "test_ts_status"],
    "laplace": ["test_lap_prior_precision", "test_lap_log_marglik", "test_lap_var_mean"],
    "maha": ["test_maha_acc1", "test_maha_mean", "test_maha_shrinkage"],
    "knn": ["test_knn_acc1", "test_knn_mean", "test_knn_k"],
    "vim": ["test_vim_acc1", "test_vim_mean", "test_vim_dim", "test_vim_alpha"],
    "conformal": ["test_cp_alpha", "test_cp_qhat", "test_cp_coverage", "test_cp_size", "test_cp_empty", "test_cp_singleton", "test_cp_sscv",
                  "test_cp_worst_class", "test_cp_n_cal"],
}
# the families every head admits, and the two that depend on the head: ViM needs affine logits, the Laplace fit its own head
EVERY = ("calibration", "set_calibration", "detection", "temperature", "maha", "knn", "conformal")
ADMITS = {"gp": EVERY, "het": EVERY, "ens": EVERY + ("vim",), "lap": EVERY + ("vim", "laplace"), "mcd": EVERY + ("vim",), "lw": EVERY + ("vim",),
          "dist": EVERY + ("vim",), "linear": EVERY + ("vim",)}
NAMES = ("gp", "het", "ens", "lap", "mcd", "lw", "dist", "linear")


def _report(head, names):
    fits = {k: v for k, v in FITS.items() if k in names}
    return rlp.report(dict(STATS), fits, head, [f for f in rlp.FAMILIES if f.name in fits], DIMS)


def test_the_tables_hold_the_heads_and_families_in_their_orders():
    assert len(rlp.HEADS) == len(NAMES) and [h.switch for h in rlp.HEADS] == ["gp_layer", "het_layer", "ensembles", "laplace", "mc_dropout_forwards",
                                                                           "learn_layer_weights", None, None]
    assert [f.name for f in rlp.FAMILIES] == ["calibration", "set_calibration", "detection", "temperature", "laplace", "maha", "knn", "vim",
                                             "conformal", "perturbations", "corruptions"]
    assert rlp.FIT_ORDER == ("calibration", "detection", "laplace", "maha", "knn", "vim", "temperature", "conformal", "set_calibration")
    assert [key for key, _ in rlp.VAR_MEAN_LINES] == ["gp_var_mean", "het_var_mean", "lap_var_mean", "dist_var_mean"]      # no ens, no mcd line
    assert [h.affine(rlp.get_args([])) for h in rlp.HEADS] == [False, False, True, True, True, True, True, True]
    assert rlp.ENS.affine(rlp.get_args(["--ens_combine", "probs"])) is False
    assert rlp.GP.logit_kw(rlp.get_args(["--gp_mean_field", "0.5"])) == {"mean_field": 0.5} and rlp.GP.logit_kw(rlp.get_args([])) == {}
    assert all(h.logit_kw(rlp.get_args(["--gp_mean_field", "0.5"])) == {} for h in rlp.HEADS[1:])
    assert rlp.given(rlp.get_args(["--knn_k", "3"]), "knn_", ("k", "temperature")) == {"k": 3}


@pytest.mark.parametrize("name", NAMES)
def test_eval_report_of_a_head_with_every_family_it_admits(name):
    head, names = rlp.HEADS[NAMES.index(name)], ADMITS[name]
    front, behind, entries = _report(head, names)
    assert front == [ln for k in ("temperature", "laplace", "maha", "knn", "vim") if k in names for ln in FRONT[k]]
    assert behind == HEAD_LINES[name] + [ln for k in ("calibration", "set_calibration", "detection", "conformal") for ln in BEHIND[k]]
    assert list(entries) == ["test_loss", "test_acc1", "test_acc5"] + LOG_KEYS["calibration"] + HEAD_KEYS[name] + [
        key for k in ("set_calibration", "detection", "temperature", "laplace", "maha", "knn", "vim", "conformal") if k in names for key in LOG_KEYS[k]]
    assert entries["test_acc1"] == 50.0 and entries["test_cp_qhat"] == [H] and entries["test_ts_temperature"] == 2.0


def test_eval_report_without_a_fit_and_without_families():
    # --ts_temperature: no line, the one entry; --eval alone: nothing beyond the three figures, so main() writes no log line
    fits = {"temperature": None}
    front, behind, entries = rlp.report(dict(STATS), fits, rlp.LINEAR, [f for f in rlp.FAMILIES if f.name in fits], DIMS)
    assert (front, behind) == ([], []) and list(entries) == ["test_loss", "test_acc1", "test_acc5", "test_ts_temperature"]
    assert rlp.report(dict(STATS), {}, rlp.LINEAR, [], DIMS) == ([], [], {"test_loss": H, "test_acc1": 50.0, "test_acc5": 75.0})


@pytest.mark.parametrize("name", NAMES)
def test_epoch_report(name):
    """A training run: the eval-only families are absent because their checks demand --eval; the Laplace probe fits with --lap_data_path."""
    head = rlp.HEADS[NAMES.index(name)]
    names = ("calibration", "set_calibration") + (("laplace",) if name == "lap" else ())
    front, behind, entries = _report(head, names)
    assert front == (FRONT["laplace"] if name == "lap" else [])
    assert behind == HEAD_LINES[name] + BEHIND["calibration"] + BEHIND["set_calibration"]
    assert list(entries) == ["test_loss", "test_acc1", "test_acc5"] + LOG_KEYS["calibration"] + HEAD_KEYS[name] + LOG_KEYS["set_calibration"] + (
        LOG_KEYS["laplace"] if name == "lap" else [])
    if name == "lap":               # --laplace without --lap_data_path trains as a linear probe: no fit, no line, no entry
        fits = {"laplace": None}
        assert rlp.report(dict(STATS), fits, head, [f for f in rlp.FAMILIES if f.name in fits], DIMS) == ([], [], {k: entries[k] for k in list(entries)[:3]})


SWITCHES = {"gp": ["--gp_layer"], "het": ["--het_layer"], "ens": ["--ensembles"], "lap": ["--laplace"],
            "mcd": ["--mc_dropout_forwards", "4", "--attn_drop_rate", "0.1"], "lw": ["--learn_layer_weights"]}
# the later head of HEADS speaks
TWO_HEADS = {
    "het": "--het_layer and --gp_layer are two heads: give one",
    "ens": "--ensembles is an ensemble of linear heads: give it without --gp_layer / --het_layer",
    "lap": "--laplace is a post-hoc fit of the linear head: give it without --gp_layer / --het_layer / --ensembles",
    "mcd": "--mc_dropout_forwards samples the linear head: give it without --gp_layer / --het_layer / --ensembles / --laplace",
    "lw": "--learn_layer_weights mixes the features of the linear head: give it without --gp_layer / --het_layer / --ensembles / --laplace / "
          "--mc_dropout_forwards",
}


@pytest.mark.parametrize("first,second", [(a, b) for i, a in enumerate(list(SWITCHES)) for b in list(SWITCHES)[i + 1:]])
def test_two_heads_are_refused_before_anything_is_loaded(first, second, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    base = ["--nb_classes", "10", "--finetune", "none.pth"]
    for flags in (SWITCHES[first] + SWITCHES[second], SWITCHES[second] + SWITCHES[first]):
        with pytest.raises(ValueError) as e:
            rlp.main(rlp.get_args(base + flags))
        assert str(e.value) == TWO_HEADS[second]
    with pytest.raises(FileNotFoundError):                      # one head alone stops at the checkpoint
        rlp.main(rlp.get_args(base + SWITCHES[second]))


def _defaults(fn, names):
    params = inspect.signature(fn).parameters
    return {n: params[n].default for n in names}


def test_library_defaults_equal_the_documented_ones():
    """What the command line passes only when given: the library's defaults are the ones the usage text names."""
    from uncertainty_vit_amd.dist_probe import DistProbe
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.lw_probe import LayerWeightedProbe
    from uncertainty_vit_amd.mcd_probe import MCDropoutProbe
    for fn, want in (
            (GPProbe.__init__, dict(num_inducing=None, kernel_scale=1.0, cov_momentum=0.999, cov_ridge_penalty=1e-3)),
            (GPProbe.evaluate, dict(mean_field=0.0)), (GPProbe.fit_temperature, dict(mean_field=0.0)), (GPProbe.fit_conformal, dict(mean_field=0.0)),
            (GPProbe.evaluate_conformal, dict(mean_field=0.0)), (GPProbe.evaluate_stability, dict(mean_field=0.0)),
            (HetProbe.__init__, dict(num_factors=10, temperature=1.0, train_mc_samples=1000, test_mc_samples=1000, seed=42)),
            (EnsembleProbe.__init__, dict(combine="logits", bagging=False, seed=0)),
            (MCDropoutProbe.__init__, dict(layers=0, combine="logits", seed=0)),
            (LayerWeightedProbe.__init__, dict(use_cls=False, layernorm_before_combine=False)),
            (DistProbe.__init__, dict(mean_field=0.0, var_scale=1.0)),
            (LinearProbe.fit_neighbours, dict(k=20, temperature=0.07)),
            (LinearProbe.fit_density, dict(shrinkage=1e-3)),
            (LinearProbe.fit_vim, dict(dim=None)),
            (LinearProbe.fit_temperature, dict(tol=1e-7, max_iter=16)),
            (LinearProbe.fit_conformal, dict(alpha=0.1, score="aps", randomized=False, seed=0)),
            (LinearProbe.enable_set_calibration, dict(ece_bins=15, cw_bins=15, ace_bins=15, tace_bins=30, tace_threshold=0.01))):
        assert _defaults(fn, want) == want, fn.__qualname__
