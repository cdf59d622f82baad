#!/usr/bin/env python
"""Linear probe of a pre-training checkpoint -- the reference's `run_class_finetuning.py --linear_classifier`, with its flag names,
types and defaults where the flags exist there:

    python run_linear_probe.py --model beit_base_patch16_224 --finetune ckpt/checkpoint-799.pth \\
        --data_set image_folder --data_path data/train --eval_data_path data/val --nb_classes 1000 --output_dir probe/
    python run_linear_probe.py --model beit_base_patch16_224 --finetune ckpt/checkpoint-799.pth --resume probe/probe-29.pth \\
        --data_set image_folder --eval_data_path data/val --nb_classes 1000 --eval

The encoder is frozen; the patch tokens of its last block (`--target_layer L`: of block L, the encoder is built with L + 1 blocks)
are mean-pooled, normalised without affine and fed to one nn.Linear, the only thing that trains (uncertainty-vit_amd/linear_probe.py).
`--finetune` is a checkpoint written by run_cyclical.py (utils.save_model); its `lm_head.*` and `mask_token` entries are loaded but
never used.  Training reads `--data_path` with flip + RandomResizedCrop (augmentation level 3), evaluation reads `--eval_data_path`
with resize + center crop (level 1), both augmented on the device.  Single GPU.  `--calibration` adds the reference's calibration
metrics to every evaluation: a second line `* ECE ... TACE ... NLL ... AUROC ...` and `test_ECE`, `test_TACE`, `test_NLL`,
`test_AUROC` in log.txt (with --eval: one entry of the test figures, when --output_dir is given).

`--set_calibration` (an addition to the reference; beside --calibration or without it) reports the calibration of the evaluation set
as a whole instead of means of per-batch values: every labelled batch's probabilities and labels go into a device store, one call
behind the last batch (csrc/setcalib.hip) gives top-label ECE, MCE and OE with the reliability table, NLL, the
Brier score and per class SCE, ACE, TACE and AUROC, all with the textbook bin accuracy.  Every evaluation prints `* Set ECE .. MCE ..
OE .. NLL .. Brier .. SCE .. ACE .. TACE .. AUROC .. on <n> images (<c> classes with an AUROC)` behind the `* Acc@1` (and `* ECE`)
line; log.txt gains `test_set_{ECE,MCE,OE,NLL,Brier,SCE,ACE,TACE,AUROC}` and `test_set_reliability`, --output_dir with --eval gains
`reliability.json`; every set of a corruption sweep gains the line and `test_c_<name>_<severity>_set_<key>`, the per-severity summary
`set-ECE .. Brier ..` and `test_c_severity_set_{ECE,NLL,Brier}`.  `--scal_ece_bins` (15), `--scal_cw_bins` (15), `--scal_ace_bins` (15),
`--scal_tace_bins` (30), `--scal_tace_threshold` (0.01) steer it and are refused without it.

`--eval --perturbation_path DIR [--perturbations NAME ...]` adds the reference's p_evaluate() behind the evaluation: every `DIR/NAME.npy`
(without --perturbations: every `DIR/*.npy`, sorted) is an (N, F, H, W, 3) uint8 array of N sequences of F frames (the CIFAR-100-P
layout).  Per perturbation the flipping probability, the top-5 distance and the Zipf distance are printed in the reference's format
and, with --output_dir, appended to log.txt as `test_flip_NAME`, `test_top5_NAME`, `test_zipf_NAME`; `Mean Flipping Prob` closes
the list.  A perturbation with `noise` in its name compares every frame with frame 0, any other with the frame before it.

`--gp_layer` (the reference's flag) replaces the nn.Linear by the reference's random-feature Gaussian-process head
(modeling_finetune.SNGP; uncertainty-vit_amd/gp_probe.py): LayerNorm, frozen random Fourier features with a cosine, a trainable
output layer and a Laplace precision matrix accumulated over the training steps.  `--gp_num_inducing D` (default: the embed dim),
`--gp_cov_momentum` (0.999; at <= 0 the precision matrix is the exact sum and is reset at the start of every epoch, so that the
data are counted once), `--gp_cov_ridge_penalty` (1e-3), `--gp_kernel_scale` (1.0).  Every evaluation then prints a line
`* GP variance mean ...` after `* Acc@1` and log.txt gains `test_gp_var_mean`, the mean predictive variance over the evaluation set.
`--gp_mean_field FACTOR` (default 0: off) evaluates on edward2's mean-field logits z / sqrt(1 + FACTOR * var), an addition to the
reference.  `--calibration` and `--perturbation_path` work with the head unchanged.

`--het_layer` (the reference's flag; exclusive with --gp_layer) replaces the nn.Linear by the heteroscedastic head the reference's
modeling_finetune.MCSoftmaxDenseFA describes (uncertainty-vit_amd/het_probe.py): the logits get a Gaussian noise with an
input-dependent low-rank-plus-diagonal covariance and the prediction is the Monte-Carlo mean of the softmax over that noise.
`--het_num_factors R` (10), `--het_temperature` (1.0), `--het_train_mc_samples` (1000), `--het_test_mc_samples` (1000), `--het_seed`
(42).  Every evaluation then prints a line `* Het variance mean ...` after `* Acc@1` and log.txt gains `test_het_var_mean`, the mean
over the evaluation set of the Monte-Carlo variance of the predicted class's probability.  `--calibration` and `--perturbation_path`
work with the head unchanged.

`--ensembles` (the reference's flag; exclusive with --gp_layer and --het_layer) trains and evaluates an ensemble of linear heads on
the one frozen encoder (uncertainty-vit_amd/ens_probe.py): the members share the encoder forward of every batch, each receives its own
gradient and its own gradient clip, and the evaluation is on their combination.  `--ens_members M` (5, at most 16), `--ens_combine
logits|probs` (`logits`: the mean of the members' logits, the reference's; `probs`: the logarithm of the mean of their softmaxes),
`--ens_bagging` (online bagging: a Poisson(1) weight per member and sample presentation; off by default, an addition to the
reference), `--ens_seed` (0).  `--eval --ens_heads A.pth B.pth ...` assembles the ensemble from the `model` entries of separately
trained linear-probe checkpoints (probe-N.pth), the reference's workflow; the member count is the number of files.  Every evaluation
then prints, after the ensemble's `* Acc@1` line, one `* Member m Acc@1 ... Acc@5 ... loss ...` line per member and
`* Ens entropy ... expected ... MI ... variance ... disagreement ...`; log.txt gains `test_member{m}_acc1`, `test_ens_total`,
`test_ens_aleatoric`, `test_ens_mi`, `test_ens_var`, `test_ens_disagreement`.  `--calibration` and `--perturbation_path` work on the
combined logits unchanged.

`--eval --detection` asks whether each per-sample uncertainty ranks the wrong predictions above the right ones: the columns `msp`
(1 - max softmax), `entropy` and `energy` (-logsumexp) of the evaluated logits, plus `gp_var`, `het_var` or the five `ens_*` columns of
the head in use, are sorted over the whole evaluation set on the device and the run prints, per column,
`* Detect misclassification <column> AUROC ... AUPR ... FPR95 ... AURC ...`.  `--ood_data_path DIR` (implies --detection) sends the
images of another data set, an image folder whose class folders are ignored, through the same forward and adds
`* Detect OOD <column> AUROC ... AUPR ... FPR95 ...` (positive = OOD image).  log.txt gains `test_mis_<column>_<metric>` and
`test_ood_<column>_<metric>`.

`--eval --ts_data_path DIR` repairs the head's calibration by post-hoc temperature scaling (Guo et al., 2017; an addition to the
reference): DIR is a labelled image folder with the evaluation's classes, read with the evaluation pipeline; one scalar T is fitted
on it on the device by minimising the NLL of softmax(z / T) (`--ts_tol`, default 1e-7, and `--ts_max_iter`, default 16, are the stopping
rule), and `--eval_data_path` is then evaluated on z / T.  The accuracy does not change; loss, the calibration metrics and the msp,
entropy and energy columns do.  Before `* Acc@1` the run prints
`* Temperature <T> NLL <before> -> <after> on <n> calibration images (<iterations> passes, <status>)` and log.txt gains
`test_ts_temperature`, `test_ts_nll_before`, `test_ts_nll_after`, `test_ts_n`, `test_ts_iterations`, `test_ts_status`.
`--ts_temperature T` applies a given T without a fit (log.txt: `test_ts_temperature` alone); the two are exclusive.

`--eval --cp_data_path DIR` calibrates split-conformal prediction sets (an addition to the reference): DIR is a labelled image folder
with the evaluation's classes (it may be the folder of --ts_data_path).  `--cp_score lac|aps|raps` (default aps; raps with
`--cp_lambda`, default 0.01, and `--cp_kreg`, default 5) scores every calibration image's label on the device, `--cp_alpha A [A ...]`
(default 0.1, up to 8 levels) takes the ceil((n + 1)(1 - A))-th smallest score as the threshold, and every evaluation image then
gets the set of classes whose score does not exceed it: the true class is in the set with probability >= 1 - A, whatever the head.
`--cp_randomized` (with `--cp_seed`, default 0) randomises the last class of an aps / raps set.  With --ts_data_path or
--ts_temperature both the calibration and the evaluation see z / T (the temperature is fitted first).  Behind the other lines the run
prints, per level, `* Conformal <score> alpha <A> qhat <q> coverage <c> size <mean> empty <e> singleton <s> SSCV <v> worst-class <w>
on <n> calibration images`, and log.txt gains `test_cp_alpha`, `test_cp_qhat`, `test_cp_coverage`, `test_cp_size`, `test_cp_empty`,
`test_cp_singleton`, `test_cp_sscv`, `test_cp_worst_class` (lists in --cp_alpha order) and `test_cp_n_cal`.

`--laplace` (the reference's flag; exclusive with --gp_layer, --het_layer and --ensembles) gives a trained linear head an epistemic
uncertainty after the fact (uncertainty-vit_amd/lap_probe.py): a last-layer K-FAC Laplace approximation whose two Kronecker factors
are accumulated on the device over `--lap_data_path DIR`, a labelled image folder read with the evaluation pipeline (required with
--eval unless `--lap_state FILE` loads a saved fit).  `--lap_prior_precision X|marglik` is the prior precision (default 1.0;
`marglik` takes the arg-max of the marginal likelihood over 97 log-spaced points of [1e-4, 1e8]).  Every evaluation then runs on
the probit-scaled logits z / sqrt(1 + pi / 8 var), in front of the temperature and the conformal calibration, which are fitted
after the Laplace fit; `--detection` gains the column `lap_var`.  Before `* Acc@1` the run prints
`* Laplace prior precision <tau> (<given|marglik[, grid edge]>) log-marglik <v> NLL <nll / n> on <n> images` and
`* Laplace variance mean <v>`; log.txt gains `test_lap_prior_precision`, `test_lap_log_marglik`, `test_lap_var_mean`; with
--output_dir the fit is saved as `laplace.pth`.  Without --eval the head trains as a linear probe and, with --lap_data_path, every
epoch's evaluation uses the fit of that epoch's head.

`--maha_data_path DIR` (with --eval; every head, also with --laplace; implies --detection) fits class-conditional Gaussians with one
tied covariance, and one background Gaussian, on the frozen features of a labelled image folder read with the evaluation pipeline
(LinearProbe.fit_density), and the detection gains the columns `maha` (the smallest squared Mahalanobis
distance to a class mean) and `rmaha` (that minus the squared distance to the background Gaussian).  `--maha_shrinkage RHO` (default
1e-3) is the shrinkage rho of Sigma + rho tr(Sigma) / C I; `--maha_state FILE` loads a saved fit instead (exclusive with
--maha_data_path; with --maha_shrinkage the saved sums are factorised again).  Before `* Acc@1` the run prints
`* Mahalanobis fit on <n> images (<skipped> skipped), <K> classes (<e> empty), shrinkage <rho>, log-det <v> background <v0>` and
`* Mahalanobis Acc@1 <a> mean <m>` (the nearest-class-mean accuracy and the mean `maha` of the evaluation set); log.txt gains
`test_maha_acc1`, `test_maha_mean`, `test_maha_shrinkage`; with --output_dir the fit is saved as `density.pth`.

`--knn_data_path DIR` (with --eval; every head, also with --laplace and --maha_*; implies --detection) stores the unit-length bf16
features of a labelled image folder, read with the evaluation pipeline, as a neighbour bank (LinearProbe.fit_neighbours, DESIGN.md
section 9.11).  The detection gains the column `knn` = 2 - 2 s_k, the squared distance to the k-th nearest bank feature (deep nearest
neighbours, Sun et al. 2022), and the run reports the weighted k-NN accuracy of DINO / iBOT, which trains nothing.  `--knn_k K`
(default 20, at most 256) and `--knn_temperature T` (default 0.07) set the neighbour count and the vote's temperature;
`--knn_state FILE` loads a saved bank instead (exclusive with --knn_data_path; --knn_k / --knn_temperature then override the saved
ones).  Before `* Acc@1` the run prints `* kNN bank of <n> images (<skipped> skipped), <K> classes, k <k>, temperature <T>` and
`* kNN Acc@1 <a> mean <m>`; log.txt gains `test_knn_acc1`, `test_knn_mean`, `test_knn_k`; with --output_dir the bank is saved as
`neighbours.pth`.

`--vim_data_path DIR` (with --eval; the linear head, --laplace and --ensembles with --ens_combine logits, also with --maha_* and
--knn_*; implies --detection) fits ViM (virtual-logit matching, Wang et al. 2022; LinearProbe.fit_vim) on
the frozen features of a labelled image folder, which is read twice (once when --maha_data_path names the same folder: the density's
moments are reused).  The detection gains the columns `vim` = alpha |R (f - o)| - logsumexp(z) and `residual` = |R (f - o)|, the
length of the feature's part outside the principal space of the training features.  `--vim_dim D` is that space's dimension
(default 1000 for C >= 2048, 512 for C >= 768, else C // 2); `--vim_state FILE` loads a saved fit instead (exclusive with
--vim_data_path).  --gp_layer, --het_layer and --ens_combine probs are refused: their logits are not affine in the feature.  Before
`* Acc@1` the run prints `* ViM fit on <n> images (<skipped> skipped), dim <D> of <C>, alpha <a>, explained <e>` and
`* ViM Acc@1 <a> mean <m>`; log.txt gains `test_vim_acc1`, `test_vim_mean`, `test_vim_dim`, `test_vim_alpha`; with --output_dir the
fit is saved as `vim.pth`.

`--mc_dropout_forwards T` (the reference's flag; 0 or absent: off; exclusive with --gp_layer, --het_layer, --ensembles and --laplace)
evaluates the linear head under MC-dropout (uncertainty-vit_amd/mcd_probe.py): every evaluated batch runs one
deterministic encoder forward and T passes under attention dropout, whose logits are combined on the device.  `--attn_drop_rate P`
(the reference's flag; required > 0 with T > 0, refused without T: every other forward of the probe is dropout-free) is the dropout
rate the encoder is built with; `--mc_dropout_layers n` applies it in
the last n blocks only (0, the default: in all of them), so that a batch costs 1 + T n / L encoder passes; `--mc_combine logits|probs`
(the mean of the passes' logits, the reference's; or the logarithm of the mean of their softmaxes); `--mc_seed` (0).  Training is the
linear probe's, on the deterministic forward.  --calibration, --detection / --ood_data_path (with the columns mcd_total,
mcd_aleatoric, mcd_mi, mcd_var, mcd_disagreement), --ts_*, --cp_*, --perturbation_path and --maha_* / --knn_* / --vim_* (on the
deterministic feature) work on the combined logits.  After `* Acc@1` the run prints `* MC-dropout passes <T> layers <n> of <L> rate
<p> entropy ... expected ... MI ... variance ... disagreement ...` and `* Deterministic Acc@1 ...`; log.txt gains
`test_mcd_{total,aleatoric,mi,var,disagreement,det_acc1,passes}`.

`--learn_layer_weights` (the reference's flag; exclusive with --gp_layer, --het_layer, --ensembles, --laplace and
--mc_dropout_forwards) probes every block at once (uncertainty-vit_amd/lw_probe.py): the encoder is built at
full depth (a given --target_layer is ignored with one printed line, as the reference does), every block's output is pooled -- the mean
over ALL its tokens, the cls token included -- and a trained softmax over `depth` scalars, `layer_log_weights`, mixes the pooled
vectors in front of the nn.Linear; no LayerNorm follows the mix.  `--layernorm_before_combine` normalises every block's pooled vector
(no affine, eps 1e-5) before the mix, `--use_cls` pools token 0 instead of the mean; both are refused without --learn_layer_weights
(the reference's --use_cls alone needs a trained final norm, which is not built).  One run replaces a sweep over --target_layer, and
the trained weights say which blocks carry the signal: every epoch and every --eval prints `* Layer weights w0 w1 ... (argmax: block
l)` after `* Acc@1`, and log.txt gains `test_layer_weights`.  Checkpoints hold `head.weight`, `head.bias` and `layer_log_weights`;
--resume refuses one without the third key or of another depth.  --calibration, --detection / --ood_data_path, --ts_*, --cp_*,
--maha_*, --knn_*, --vim_* and --perturbation_path work unchanged on the mixed feature and its logits.

`--eval --corruptions NAME ... | all | full` (with --eval_data_path) adds the reference's c_evaluate() behind the evaluation, on corruptions
generated on the device (uncertainty-vit_amd/corruptions.py): the clean evaluation images are decoded once and
kept on the device as uint8 (`--corruption_cache_images N`, default 65536; a larger folder is read again per set), and every
(corruption, severity) set -- gaussian_noise, speckle_noise, impulse_noise, shot_noise, brightness, saturate, contrast, gaussian_blur,
defocus_blur (`all`: these nine) and pixelate, jpeg_compression, motion_blur, zoom_blur (uncertainty-vit_amd/corruptions_ext.py, section
9.18; `full`: the nine followed by these four) at `--corruption_severities` (default 1 2 3 4 5), noise and motion_blur's direction
seeded by `--corruption_seed` (default 0) -- is one evaluation with the run's own switches.  The constants are ImageNet-C's as
remembered, unverified, and jpeg_compression, motion_blur and zoom_blur are this project's definitions, not libjpeg's, ImageMagick's or
scipy's bytes: the figures are ImageNet-C-style, not the published benchmark.  `--corruption_path DIR` (exclusive with --corruptions) reads a pre-made tree DIR/<distortion>/<severity>/<class>/... with
the evaluation pipeline instead: the reference's DISTORTIONS order first, then the other sub-folders sorted; a missing severity folder
is an error.  The run prints `Corrupted dataset evaluation :`, `Distortion : <name>`, per severity `* Acc@1 ... CE ... ` (followed by
the set's calibration line, variance mean and detection lines when the run has them), `mCE (unnormalized) (%): ..., acc :...` and
`* Severity s Acc@1 ... CE ... rel-CE ... [ECE ... NLL ...]` per severity; log.txt gains `test_c_<name>_<severity>_<key>` per set and
`test_c_mce`, `test_c_acc`, `test_c_severity_*` (lists).

A `--model` that builds the two-stream (mean, covariance) encoder (`dist_beit_base_patch16_224`, `dist_beit_large_patch16_224`) is
probed by uncertainty-vit_amd/dist_probe.py: the nn.Linear reads the mean stream's pooled feature and trains
as the linear probe does; the covariance stream's pooled feature c gives a feature variance v = S (ELU(c) + 1) (`--dist_var_scale S`,
default 1.0) and, through the head, a variance per logit.  `--dist_mean_field FACTOR` (default 0: the reference's logits; pi / 8 =
0.3927 is the literature's value) evaluates on z / sqrt(1 + FACTOR * var); both flags are refused with a base model.  Every
evaluation prints `* Dist variance mean <v> trace mean <t>` after `* Acc@1`, log.txt gains `test_dist_var_mean` and
`test_dist_trace_mean`, and `--detection` gains the columns `dist_var` and `dist_trace`.  --calibration, --ts_*, --cp_*, --maha_*,
--knn_*, --perturbation_path, --corruptions and --target_layer work as with a base model, --vim_* at FACTOR = 0; the other heads
(--gp_layer, --het_layer, --ensembles, --laplace, --mc_dropout_forwards, --learn_layer_weights) refuse a two-stream encoder.

`--mixup A`, `--cutmix A`, `--cutmix_minmax LO HI`, `--mixup_prob`, `--mixup_switch_prob`, `--mixup_mode batch|pair|elem`, `--reprob P`,
`--remode const|rand|pixel`, `--recount N` (the reference's flags; absent = off, the reference's default --reprob 0.25 is not adopted)
erase and mix every training batch on the device in front of the encoder (uncertainty-vit_amd/probe_mix.py, csrc/mixup.hip, DESIGN.md
section 9.20) and train on the soft-target cross-entropy of the two labels of every row; the run prints `Mixup is activated!` and
log.txt's `train_loss` is that loss.  `--mix_seed` (default: --seed) seeds the draws, which depend on (seed, step) alone.  Every head
but --ensembles takes them; --eval refuses them.  Evaluation is untouched.

`--aa CONFIG` (the reference's flag, timm's string: `rand-m9-mstd0.5-inc1` is the reference's default; absent = off, that default is
not adopted) runs RandAugment on every training batch on the device, in front of the erasing and mixing and of the encoder
(uncertainty-vit_amd/probe_randaug.py, csrc/randaug.hip): per image `n` of timm's fifteen ops, each applied
with probability 0.5 at a magnitude drawn around `m`, computed as Pillow computes them, bit for bit.  `--aa_interpolation
bicubic|bilinear|nearest|random` (default bicubic, what the reference's --train_interpolation hands timm) is the filter of the affine
ops.  The draws take --mix_seed (default: --seed) and depend on (seed, step) alone.  The run prints `RandAugment is activated: ...`
with the parsed config; log.txt's `train_loss` keeps its meaning.  Every head takes it, --ensembles too; --eval refuses it.  Only
`rand` configs are built: `original`, `v0`, `augmix` and the weighted choice `w` are refused.
"""
import argparse
import json
import math
import os
import sys
import time
from dataclasses import dataclass
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from uncertainty_vit_amd.corruptions import CORRUPTIONS, DEFAULT_CACHE_IMAGES, CleanCache, CorruptedSet
from uncertainty_vit_amd.corruptions_ext import CORRUPTIONS_EXT
from uncertainty_vit_amd.datasets import FOLDER_DATA_SETS, BEiTAugment, ImageFolderPretrain, PerturbationSequences, collate_packed, collate_sequences
from uncertainty_vit_amd.engine_for_cyclical import DevicePrefetcher
from uncertainty_vit_amd import dist_probe, ens_probe, gp_probe, het_probe, lap_probe, linear_probe, lw_probe, mcd_probe, probe_mix, probe_randaug, utils


def get_args(argv=None):
    p = argparse.ArgumentParser("linear probe on the frozen encoder", add_help=True)
    a = p.add_argument
    a("--batch_size", default=64, type=int)
    a("--epochs", default=30, type=int)
    a("--model", default="deit_base_patch16_224", type=str, metavar="MODEL")
    a("--input_size", default=224, type=int)
    a("--clip_grad", type=float, default=None, metavar="NORM")
    a("--weight_decay", type=float, default=0.05)
    a("--lr", type=float, default=5e-4, metavar="LR")
    a("--min_lr", type=float, default=1e-6, metavar="LR")
    a("--warmup_epochs", type=int, default=5, metavar="N")
    a("--smoothing", type=float, default=0.1)
    a("--finetune", default="", help="pre-training checkpoint to probe")
    a("--model_key", default="model|module", type=str)
    a("--model_prefix", default="", type=str)
    a("--target_layer", default=-1, type=int, help="target output layer (0-based)")
    a("--data_path", default="/datasets01/imagenet_full_size/061417/", type=str)
    a("--eval_data_path", default=None, type=str)
    a("--nb_classes", default=0, type=int)
    a("--imagenet_default_mean_and_std", default=False, action="store_true")
    a("--data_set", default="IMNET", choices=["CIFAR100", "CIFAR10", "IMNET", "image_folder", "tiny_IMNET"], type=str)
    a("--output_dir", default="")
    a("--seed", default=0, type=int)
    a("--resume", default="", help="head checkpoint (probe-*.pth) to continue from or to evaluate")
    a("--eval", action="store_true", help="Perform evaluation only")
    a("--num_workers", default=0, type=int)
    # absent unless given (SUPPRESS): without the flag the parsed arguments, and so the first line printed, are what they were
    a("--calibration", action="store_true", default=argparse.SUPPRESS,
      help="also report ECE, TACE, NLL and AUROC of the evaluation (the reference's evaluate() beside Acc@1 / Acc@5)")
    a("--set_calibration", action="store_true", default=argparse.SUPPRESS,
      help="also report the calibration of the evaluation set as a whole: ECE, MCE, OE, NLL, Brier, SCE, ACE, TACE and per-class AUROC "
           "from one set-level call on the device (textbook bin accuracies), with the reliability table")
    a("--scal_ece_bins", type=int, default=argparse.SUPPRESS, metavar="N", help="with --set_calibration: top-label bins, 1 .. 64 (default 15)")
    a("--scal_cw_bins", type=int, default=argparse.SUPPRESS, metavar="N", help="with --set_calibration: SCE's bins per class, 1 .. 64 (default 15)")
    a("--scal_ace_bins", type=int, default=argparse.SUPPRESS, metavar="N", help="with --set_calibration: ACE's adaptive bins, 1 .. 64 (default 15)")
    a("--scal_tace_bins", type=int, default=argparse.SUPPRESS, metavar="N", help="with --set_calibration: TACE's adaptive bins, 1 .. 64 (default 30)")
    a("--scal_tace_threshold", type=float, default=argparse.SUPPRESS, metavar="T",
      help="with --set_calibration: probabilities under T count as 0 in TACE (default 0.01)")
    a("--perturbation_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="with --eval: directory of perturbation sequences, NAME.npy of shape (N, F, H, W, 3) uint8 (the reference's p_evaluate())")
    a("--perturbations", type=str, nargs="+", default=argparse.SUPPRESS, metavar="NAME",
      help="the perturbations to evaluate (default: every *.npy of --perturbation_path, sorted)")
    a("--gp_layer", action="store_true", default=argparse.SUPPRESS,
      help="probe with the reference's random-feature Gaussian-process head (modeling_finetune.SNGP) instead of the nn.Linear")
    a("--gp_num_inducing", type=int, default=argparse.SUPPRESS, metavar="D", help="random features of the GP head (default: the embed dim)")
    a("--gp_cov_momentum", type=float, default=argparse.SUPPRESS,
      help="momentum of the precision matrix (default 0.999); <= 0: the exact sum, reset at the start of every epoch")
    a("--gp_cov_ridge_penalty", type=float, default=argparse.SUPPRESS, help="ridge penalty of the precision matrix (default 1e-3)")
    a("--gp_kernel_scale", type=float, default=argparse.SUPPRESS, help="the cosine is multiplied by 1 / sqrt(this) (default 1.0)")
    a("--gp_mean_field", type=float, default=argparse.SUPPRESS, metavar="FACTOR",
      help="evaluate on the mean-field logits z / sqrt(1 + FACTOR * var) (edward2's mean_field_logits; default 0: off)")
    a("--het_layer", action="store_true", default=argparse.SUPPRESS,
      help="probe with the heteroscedastic head (modeling_finetune.MCSoftmaxDenseFA: Monte-Carlo softmax, low-rank logit noise)")
    a("--het_num_factors", type=int, default=argparse.SUPPRESS, metavar="R", help="rank of the noise covariance's low-rank part (default 10)")
    a("--het_temperature", type=float, default=argparse.SUPPRESS, help="softmax temperature of the Monte-Carlo samples (default 1.0)")
    a("--het_train_mc_samples", type=int, default=argparse.SUPPRESS, help="Monte-Carlo samples of a training step (default 1000)")
    a("--het_test_mc_samples", type=int, default=argparse.SUPPRESS, help="Monte-Carlo samples of an evaluation (default 1000)")
    a("--het_seed", type=int, default=argparse.SUPPRESS, help="seed of the noise (default 42, what the reference re-seeds with)")
    a("--ensembles", action="store_true", default=argparse.SUPPRESS,
      help="probe with an ensemble of linear heads on the one frozen encoder and evaluate their combination (the reference's flag)")
    a("--ens_members", type=int, default=argparse.SUPPRESS, metavar="M", help="members of the ensemble (default 5, at most 16)")
    a("--ens_combine", type=str, choices=["logits", "probs"], default=argparse.SUPPRESS,
      help="logits: the mean of the members' logits (default, the reference's); probs: the logarithm of the mean of their softmaxes")
    a("--ens_bagging", action="store_true", default=argparse.SUPPRESS,
      help="online bagging: a Poisson(1) weight per member and sample presentation (default: every member sees every sample once)")
    a("--ens_seed", type=int, default=argparse.SUPPRESS, help="seed of the bagging weights (default 0)")
    a("--ens_heads", type=str, nargs="+", default=argparse.SUPPRESS, metavar="PTH",
      help="with --eval: assemble the ensemble from separately trained linear-probe checkpoints (probe-N.pth); sets the member count")
    a("--detection", action="store_true", default=argparse.SUPPRESS,
      help="with --eval: does each uncertainty column rank the wrong predictions above the right ones (AUROC, AUPR, FPR95, AURC over the set)")
    a("--ood_data_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="with --eval: image folder of another data set (its class folders are ignored); adds the OOD detection metrics, implies --detection")
    a("--ts_data_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="with --eval: labelled image folder (the evaluation's classes) on which a post-hoc temperature is fitted before the evaluation")
    a("--ts_temperature", type=float, default=argparse.SUPPRESS, metavar="T",
      help="with --eval: evaluate on logits / T for this T, without a fit (exclusive with --ts_data_path)")
    a("--ts_tol", type=float, default=argparse.SUPPRESS, help="relative step at which the temperature fit stops (default 1e-7)")
    a("--ts_max_iter", type=int, default=argparse.SUPPRESS, help="passes over the calibration set the fit may take (default 16, at most 64)")
    a("--cp_data_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="with --eval: labelled image folder (the evaluation's classes) on which conformal prediction sets are calibrated")
    a("--cp_alpha", type=float, nargs="+", default=argparse.SUPPRESS, metavar="A",
      help="miscoverage levels of the conformal sets, up to 8 (default 0.1): a set holds the true class with probability >= 1 - A")
    a("--cp_score", type=str, choices=["lac", "aps", "raps"], default=argparse.SUPPRESS, help="the conformal score (default aps)")
    a("--cp_lambda", type=float, default=argparse.SUPPRESS, help="raps: the penalty per rank beyond --cp_kreg (default 0.01)")
    a("--cp_kreg", type=int, default=argparse.SUPPRESS, help="raps: the ranks that carry no penalty (default 5)")
    a("--cp_randomized", action="store_true", default=argparse.SUPPRESS,
      help="aps / raps: randomise the last class of a set with a per-image u from a seeded device generator")
    a("--cp_seed", type=int, default=argparse.SUPPRESS, help="seed of --cp_randomized (default 0)")
    a("--laplace", action="store_true", default=argparse.SUPPRESS,
      help="post-hoc last-layer K-FAC Laplace approximation of the linear head (the reference's flag): probit-scaled logits, lap_var")
    a("--lap_data_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="labelled image folder (the evaluation's classes) the Laplace factors are accumulated on, read with the evaluation pipeline")
    a("--lap_prior_precision", type=str, default=argparse.SUPPRESS, metavar="X|marglik",
      help="prior precision tau: a positive number (default 1.0) or `marglik`, the arg-max of the marginal likelihood over a grid")
    a("--lap_state", type=str, default=argparse.SUPPRESS, metavar="FILE",
      help="with --eval: load a saved Laplace fit (laplace.pth) instead of fitting")
    a("--maha_data_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="with --eval: labelled image folder (the evaluation's classes) on whose features the Mahalanobis density is fitted; adds the "
           "detection columns maha and rmaha, implies --detection")
    a("--maha_shrinkage", type=float, default=argparse.SUPPRESS, metavar="RHO",
      help="shrinkage of the two covariances, Sigma + RHO tr(Sigma) / C I (default 1e-3)")
    a("--maha_state", type=str, default=argparse.SUPPRESS, metavar="FILE",
      help="with --eval: load a saved Mahalanobis fit (density.pth) instead of fitting (exclusive with --maha_data_path)")
    a("--knn_data_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="with --eval: labelled image folder (the evaluation's classes) whose features become the neighbour bank; adds the detection "
           "column knn and the weighted k-NN accuracy, implies --detection")
    a("--knn_state", type=str, default=argparse.SUPPRESS, metavar="FILE",
      help="with --eval: load a saved neighbour bank (neighbours.pth) instead of fitting (exclusive with --knn_data_path)")
    a("--knn_k", type=int, default=argparse.SUPPRESS, metavar="K", help="neighbours per query, 1 .. 256 (default 20)")
    a("--knn_temperature", type=float, default=argparse.SUPPRESS, metavar="T",
      help="temperature of the k-NN vote exp((s_j - s_1) / T) (default 0.07)")
    a("--vim_data_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="with --eval: labelled image folder (the evaluation's classes) on whose features ViM is fitted (read twice); adds the "
           "detection columns vim and residual, implies --detection")
    a("--vim_dim", type=int, default=argparse.SUPPRESS, metavar="D",
      help="dimension of the principal space, 1 .. C - 1 (default 1000 for C >= 2048, 512 for C >= 768, else C // 2)")
    a("--vim_state", type=str, default=argparse.SUPPRESS, metavar="FILE",
      help="with --eval: load a saved ViM fit (vim.pth) instead of fitting (exclusive with --vim_data_path)")
    a("--mc_dropout_forwards", type=int, default=argparse.SUPPRESS, metavar="T",
      help="evaluate under MC-dropout: T stochastic passes per batch, combined on the device (0: off); needs --attn_drop_rate > 0")
    a("--attn_drop_rate", type=float, default=argparse.SUPPRESS, metavar="P", help="with --mc_dropout_forwards: attention dropout rate of the passes, > 0")
    a("--mc_dropout_layers", type=int, default=argparse.SUPPRESS, metavar="N",
      help="MC-dropout in the last N blocks only: 1 + T N / L encoder passes per batch (default 0: every block)")
    a("--mc_combine", type=str, choices=["logits", "probs"], default=argparse.SUPPRESS,
      help="combined logits: the mean of the passes' logits (default, the reference's) or the log of the mean of their softmaxes")
    a("--mc_seed", type=int, default=argparse.SUPPRESS, help="seed of the dropout masks (default 0)")
    a("--learn_layer_weights", action="store_true", default=argparse.SUPPRESS,
      help="pool every block's output and train a softmax over `depth` scalars that mixes them in front of the head; supersedes --target_layer")
    a("--layernorm_before_combine", action="store_true", default=argparse.SUPPRESS,
      help="with --learn_layer_weights: LayerNorm (no affine, eps 1e-5) of every block's pooled vector before the mix")
    a("--use_cls", action="store_true", default=argparse.SUPPRESS,
      help="with --learn_layer_weights: pool the cls token of every block instead of the mean over all its tokens")
    a("--dist_mean_field", type=float, default=argparse.SUPPRESS, metavar="FACTOR",
      help="two-stream --model: evaluate on z / sqrt(1 + FACTOR * var), var from the covariance stream (default 0: the reference's "
           "logits; pi / 8 = 0.3927 is the literature's value)")
    a("--dist_var_scale", type=float, default=argparse.SUPPRESS, metavar="S",
      help="two-stream --model: the scale s of the feature variance v = s (ELU(c) + 1) (default 1.0)")
    a("--corruptions", type=str, nargs="+", default=argparse.SUPPRESS, metavar="NAME",
      help="with --eval and --eval_data_path: evaluate under these corruptions of the clean evaluation images, generated on the device "
           "(names of uncertainty_vit_amd.corruptions.CORRUPTIONS and corruptions_ext.CORRUPTIONS_EXT, or `all`: the former, or `full`: "
           "both); the reference's c_evaluate()")
    a("--corruption_severities", type=int, nargs="+", default=argparse.SUPPRESS, metavar="S", help="the severities to sweep, a subset of 1 .. 5 (default: all five)")
    a("--corruption_seed", type=int, default=argparse.SUPPRESS, help="seed of the noise corruptions (default 0)")
    a("--corruption_cache_images", type=int, default=argparse.SUPPRESS, metavar="N",
      help="keep up to N clean evaluation images on the device as uint8 across the sets (default 65536); a larger folder is read again per set")
    a("--corruption_path", type=str, default=argparse.SUPPRESS, metavar="DIR",
      help="with --eval: a pre-made corrupted data set DIR/<distortion>/<severity>/<class>/... (the reference's layout), every folder read "
           "with the evaluation pipeline; exclusive with --corruptions")
    # the reference's mixup / cutmix / random-erasing flags (run_class_finetuning.py:128-149); absent = off: its own default
    # --reprob 0.25 is NOT adopted, a run without these flags trains as it always has
    a("--reprob", type=float, default=argparse.SUPPRESS, metavar="PCT", help="random erase probability per training sample (default 0: off)")
    a("--remode", type=str, default=argparse.SUPPRESS, help="random erase fill: const, rand or pixel (default pixel)")
    a("--recount", type=int, default=argparse.SUPPRESS, help="random erase boxes per erased sample, 1 .. 8 (default 1)")
    a("--mixup", type=float, default=argparse.SUPPRESS, help="mixup alpha, enabled if > 0 (default 0)")
    a("--cutmix", type=float, default=argparse.SUPPRESS, help="cutmix alpha, enabled if > 0 (default 0)")
    a("--cutmix_minmax", type=float, nargs="+", default=argparse.SUPPRESS,
      help="cutmix min / max side ratio, two values in (0, 1] ascending; overrides the alpha and enables cutmix")
    a("--mixup_prob", type=float, default=argparse.SUPPRESS, help="probability of mixing a batch (or a row) when either is enabled (default 1.0)")
    a("--mixup_switch_prob", type=float, default=argparse.SUPPRESS, help="probability of cutmix when both are enabled (default 0.5)")
    a("--mixup_mode", type=str, default=argparse.SUPPRESS, help="how the parameters are drawn: batch, pair or elem (default batch)")
    a("--mix_seed", type=int, default=argparse.SUPPRESS, help="seed of the mixing, erasing and RandAugment draws (default: --seed)")
    # the reference's --aa (run_class_finetuning.py:117); absent = off: its default rand-m9-mstd0.5-inc1 is NOT adopted
    a("--aa", type=str, default=argparse.SUPPRESS, metavar="CONFIG",
      help="RandAugment of the training batches on the device, timm's config string, e.g. rand-m9-mstd0.5-inc1 (default: off)")
    a("--aa_interpolation", type=str, default=argparse.SUPPRESS, help="filter of RandAugment's affine ops: bicubic, bilinear, nearest or random (default bicubic)")
    return p.parse_args(argv)


def given(args, prefix, names):
    """{name: args.<prefix><name>} of the names whose flag was given: the others keep the default of the library call they go to."""
    return {n: getattr(args, prefix + n) for n in names if hasattr(args, prefix + n)}


def append_log(output_dir, entries):
    with open(os.path.join(output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
        f.write(json.dumps(entries) + "\n")


CALIB_KEYS = ("ECE", "TACE", "NLL", "AUROC")
GP_FLAGS = ("gp_num_inducing", "gp_cov_momentum", "gp_cov_ridge_penalty", "gp_kernel_scale", "gp_mean_field")
HET_FLAGS = ("het_num_factors", "het_temperature", "het_train_mc_samples", "het_test_mc_samples", "het_seed")
ENS_FLAGS = ("ens_members", "ens_combine", "ens_bagging", "ens_seed", "ens_heads")
ENS_KEYS = ("ens_total", "ens_aleatoric", "ens_mi", "ens_var", "ens_disagreement")
MCD_FLAGS = ("mc_dropout_layers", "mc_combine", "mc_seed")
MCD_KEYS = ("mcd_total", "mcd_aleatoric", "mcd_mi", "mcd_var", "mcd_disagreement")


def calibration_line(stats):
    return "* ECE {ECE:.5f} TACE {TACE:.5f} NLL {NLL:.5f} AUROC {AUROC:.5f}".format(**stats)


SCAL_FLAGS = ("scal_ece_bins", "scal_cw_bins", "scal_ace_bins", "scal_tace_bins", "scal_tace_threshold")
SCAL_LINE_KEYS = ("ECE", "MCE", "OE", "NLL", "Brier", "SCE", "ACE", "TACE", "AUROC")
SCAL_SUMMARY_KEYS = ("ECE", "NLL", "Brier")


MIX_FLAGS = {"mixup": "mixup_alpha", "cutmix": "cutmix_alpha", "cutmix_minmax": "cutmix_minmax", "mixup_prob": "prob",
             "mixup_switch_prob": "switch_prob", "mixup_mode": "mode", "reprob": "reprob", "remode": "remode", "recount": "recount"}


def build_mixer(args):
    """The probe_mix.BatchMixer of the mixup / cutmix / random-erasing flags, or None when none of them switches anything on.  Refused
    (ValueError): a value outside its range (BatchMixer's own checks), and an active mixer beside --eval or --ensembles."""
    kw = {name: getattr(args, flag) for flag, name in MIX_FLAGS.items() if hasattr(args, flag)}
    mixer = probe_mix.BatchMixer(seed=getattr(args, "mix_seed", args.seed), **kw)
    if not mixer.enabled:
        return None
    if args.eval:
        raise ValueError("--mixup / --cutmix / --cutmix_minmax / --reprob change the training batches: give them without --eval")
    if getattr(args, "ensembles", False):
        raise ValueError("--mixup / --cutmix / --cutmix_minmax / --reprob are not built under --ensembles: its loss is the members' "
                         "bagged cross-entropy (uvit_op_ens_ce)")
    return mixer


def build_augmenter(args):
    """The probe_randaug.RandAugmenter of --aa / --aa_interpolation, or None without --aa.  Refused (ValueError, NotImplementedError): a
    config that is not a `rand` one or cannot be read, an unknown interpolation, --aa_interpolation without --aa, and --aa beside --eval."""
    if not hasattr(args, "aa"):
        if hasattr(args, "aa_interpolation"):
            raise ValueError("--aa_interpolation steers --aa: give --aa CONFIG")
        return None
    norm = BEiTAugment(args.input_size, 1, "bicubic", args.imagenet_default_mean_and_std)       # the normalisation of build_loader's batches
    aug = probe_randaug.RandAugmenter(args.aa, norm.mean, getattr(args, "aa_interpolation", "bicubic"), getattr(args, "mix_seed", args.seed),
                                      std=norm.std)
    if args.eval:
        raise ValueError("--aa changes the training batches: give it without --eval")
    return aug


def check_scal_flags(args):
    """The settings of --set_calibration (a dict for enable_set_calibration), or None without the flag; the --scal_* flags steer it
    and are refused without it, as is a value outside the kernels' limits."""
    given = [f for f in SCAL_FLAGS if hasattr(args, f)]
    if not getattr(args, "set_calibration", False):
        if given:
            raise ValueError("--" + " / --".join(given) + " steer the set-level calibration: give --set_calibration")
        return None
    out = {f[len("scal_"):]: getattr(args, f) for f in given}
    for k, v in out.items():
        if k.endswith("_bins") and not 1 <= v <= 64:
            raise ValueError(f"--scal_{k} must be in 1 .. 64, got {v}")
    if not 0.0 <= out.get("tace_threshold", 0.01) <= 1.0:
        raise ValueError(f"--scal_tace_threshold must be in [0, 1], got {out['tace_threshold']}")
    return out


def set_calibration_line(sc):
    return ("* Set ECE {ECE:.5f} MCE {MCE:.5f} OE {OE:.5f} NLL {NLL:.5f} Brier {Brier:.5f} SCE {SCE:.5f} ACE {ACE:.5f} TACE {TACE:.5f} "
            "AUROC {AUROC:.5f} on {n} images ({auroc_classes} classes with an AUROC)").format(**sc)


def set_calibration_log_entries(sc, prefix="test_set_"):
    """What log.txt gains: the nine set-level numbers and, for the evaluation itself, the reliability table [[prop, acc, conf], ...]."""
    out = {prefix + k: sc[k] for k in SCAL_LINE_KEYS}
    if prefix == "test_set_":
        out["test_set_reliability"] = sc["reliability"]
    return out


def write_reliability(output_dir, sc):
    """reliability.json: the bin table and the per-class arrays of the evaluation."""
    with open(os.path.join(output_dir, "reliability.json"), mode="w", encoding="utf-8") as f:
        json.dump({"n": sc["n"], "n_bad": sc["n_bad"], "reliability": sc["reliability"], "per_class": sc["per_class"]}, f)
        f.write("\n")


def gp_variance_line(stats):
    return "* GP variance mean {gp_var_mean:.6f}".format(**stats)


def het_variance_line(stats):
    return "* Het variance mean {het_var_mean:.6f}".format(**stats)


def ens_member_count(args):
    """Members of the ensemble: the number of --ens_heads files when given, else --ens_members (5)."""
    heads = getattr(args, "ens_heads", None)
    return len(heads) if heads is not None else getattr(args, "ens_members", 5)


def ens_lines(stats):
    """One line per member, then the entropy split of the ensemble."""
    rows = zip(stats["member_acc1"], stats["member_acc5"], stats["member_loss"])
    lines = [f"* Member {m} Acc@1 {a1:.3f} Acc@5 {a5:.3f} loss {loss:.3f}" for m, (a1, a5, loss) in enumerate(rows)]
    lines.append("* Ens entropy {ens_total:.5f} expected {ens_aleatoric:.5f} MI {ens_mi:.5f} variance {ens_var:.6f} "
                 "disagreement {ens_disagreement:.5f}".format(**stats))
    return lines


DIST_FLAGS = ("dist_mean_field", "dist_var_scale")


def check_dist_flags(args, two_stream):
    """The two-stream probe's constructor options {mean_field, var_scale} (`two_stream`: --model built a two-stream encoder), None for
    a base model.  The --dist_* flags belong to a two-stream model; the factor is finite and >= 0, the scale finite and > 0; ViM needs
    logits that are affine in the feature, which a factor > 0 ends."""
    if not two_stream:
        if any(hasattr(args, k) for k in DIST_FLAGS):
            raise ValueError("--dist_mean_field / --dist_var_scale read the covariance stream: give a two-stream --model (dist_beit_*)")
        return None
    factor, scale = getattr(args, "dist_mean_field", 0.0), getattr(args, "dist_var_scale", 1.0)
    if not 0.0 <= factor < math.inf:
        raise ValueError(f"--dist_mean_field must be finite and >= 0, got {factor}")
    if not 0.0 < scale < math.inf:
        raise ValueError(f"--dist_var_scale must be finite and > 0, got {scale}")
    if factor and any(hasattr(args, k) for k in VIM_FLAGS):
        raise ValueError("--vim_* need logits that are affine in the feature: not with --dist_mean_field > 0")
    return {"mean_field": factor, "var_scale": scale}


def dist_variance_line(stats):
    return "* Dist variance mean {dist_var_mean:.6f} trace mean {dist_trace_mean:.6f}".format(**stats)


def check_mcd_flags(args):
    """The number of MC-dropout passes (--mc_dropout_forwards; 0: off).  The --mc_* flags and --attn_drop_rate belong to it, it needs a rate > 0,
    and it samples the linear head: the heads in front of it in HEADS are other heads (check_head)."""
    T = getattr(args, "mc_dropout_forwards", 0)
    if T < 0:
        raise ValueError(f"--mc_dropout_forwards must be >= 0, got {T}")
    if not check_head(MCD, args):
        return 0
    if not getattr(args, "attn_drop_rate", 0.0) > 0.0:
        raise ValueError("--mc_dropout_forwards samples the attention dropout: give --attn_drop_rate P > 0")
    if getattr(args, "mc_dropout_layers", 0) < 0:
        raise ValueError(f"--mc_dropout_layers must be >= 0, got {args.mc_dropout_layers}")
    return T


def check_lw_flags(args):
    """Whether the run learns layer weights (--learn_layer_weights).  --layernorm_before_combine and --use_cls belong to it; it mixes
    the features of the linear head: the heads in front of it in HEADS are other heads (check_head)."""
    return check_head(LW, args)


def layer_weights_line(weights):
    """The line behind `* Acc@1`: softmax(layer_log_weights) in block order and the block with the largest weight."""
    return "* Layer weights {} (argmax: block {})".format(" ".join(f"{w:.4f}" for w in weights), max(range(len(weights)), key=weights.__getitem__))


def mcd_lines(stats, depth, rate):
    """The two lines behind `* Acc@1`: the entropy split of the passes, and the accuracy of the deterministic pass."""
    return ["* MC-dropout passes {mcd_passes} layers {mcd_layers} of {depth} rate {rate:g} entropy {mcd_total:.5f} expected "
            "{mcd_aleatoric:.5f} MI {mcd_mi:.5f} variance {mcd_var:.6f} disagreement {mcd_disagreement:.5f}".format(depth=depth, rate=rate, **stats),
            "* Deterministic Acc@1 {det_acc1:.3f}".format(**stats)]


def mcd_log_entries(stats):
    """What log.txt gains under MC-dropout: the five means, the deterministic accuracy and the number of passes."""
    out = {f"test_{k}": stats[k] for k in MCD_KEYS}
    out.update(test_mcd_det_acc1=stats["det_acc1"], test_mcd_passes=stats["mcd_passes"])
    return out


def ens_log_entries(stats):
    """What log.txt gains for an ensemble: every member's top-1 accuracy and the five means."""
    out = {f"test_member{m}_acc1": v for m, v in enumerate(stats["member_acc1"])}
    out.update({f"test_{k}": stats[k] for k in ENS_KEYS})
    return out


def check_detection_flags(args):
    """Whether the run computes the detection metrics: --detection or --ood_data_path (which implies it); both belong to --eval."""
    want = getattr(args, "detection", False) or hasattr(args, "ood_data_path")
    if want and not args.eval:
        raise ValueError("--detection / --ood_data_path belong to an evaluation: give --eval")
    return bool(want)


TS_FLAGS = ("ts_data_path", "ts_temperature", "ts_tol", "ts_max_iter")


def check_ts_flags(args):
    """Whether the run scales its logits by a post-hoc temperature: "fit" (--ts_data_path), "given" (--ts_temperature) or None.  All
    four --ts_* flags belong to --eval; the two sources of T are exclusive and the stopping rule belongs to the fit."""
    given = [k for k in TS_FLAGS if hasattr(args, k)]
    if not given:
        return None
    if not args.eval:
        raise ValueError("--ts_data_path / --ts_temperature / --ts_tol / --ts_max_iter belong to an evaluation: give --eval")
    if hasattr(args, "ts_data_path") and hasattr(args, "ts_temperature"):
        raise ValueError("--ts_data_path fits the temperature and --ts_temperature names it: give one (with --eval)")
    if hasattr(args, "ts_data_path"):
        return "fit"
    if hasattr(args, "ts_temperature"):
        return "given"
    raise ValueError("--ts_tol / --ts_max_iter steer the fit of --eval --ts_data_path DIR: give it")


def temperature_line(fit):
    """The line in front of `* Acc@1`, from fit_temperature's result."""
    word = linear_probe.TS_STATUS[fit["status"]] if 0 <= fit["status"] < len(linear_probe.TS_STATUS) else "failed"
    return "* Temperature {T:.5f} NLL {nll_before:.5f} -> {nll_after:.5f} on {n} calibration images ({iterations} passes, {0})".format(word, **fit)


def temperature_log_entries(stats, fit=None):
    """What log.txt gains: the temperature applied and, when it was fitted, the fit's figures."""
    out = {"test_ts_temperature": stats["temperature"]}
    if fit is not None:
        out.update(test_ts_nll_before=fit["nll_before"], test_ts_nll_after=fit["nll_after"], test_ts_n=fit["n"],
                   test_ts_iterations=fit["iterations"], test_ts_status=fit["status"])
    return out


CP_FLAGS = ("cp_data_path", "cp_alpha", "cp_score", "cp_lambda", "cp_kreg", "cp_randomized", "cp_seed")


def check_cp_flags(args):
    """Whether the run calibrates and reports conformal sets (--cp_data_path).  All --cp_* flags belong to --eval, every other one
    needs --cp_data_path, and --cp_lambda / --cp_kreg belong to --cp_score raps."""
    given = [k for k in CP_FLAGS if hasattr(args, k)]
    if not given:
        return False
    if not args.eval:
        raise ValueError("the --cp_* flags belong to an evaluation: give --eval")
    if not hasattr(args, "cp_data_path"):
        raise ValueError("--cp_alpha / --cp_score / --cp_lambda / --cp_kreg / --cp_randomized / --cp_seed steer the conformal calibration "
                         "of --eval --cp_data_path DIR: give it")
    if (hasattr(args, "cp_lambda") or hasattr(args, "cp_kreg")) and getattr(args, "cp_score", "aps") != "raps":
        raise ValueError("--cp_lambda / --cp_kreg are the penalty of --cp_score raps: give it")
    return True


LAP_FLAGS = ("lap_data_path", "lap_prior_precision", "lap_state")


def lap_prior_precision(args):
    """--lap_prior_precision as fit_laplace takes it: "marglik" or a positive number; None when the flag is absent."""
    v = getattr(args, "lap_prior_precision", None)
    if v is None or v == "marglik":
        return v
    try:
        tau = float(v)
    except ValueError:
        tau = float("nan")
    if not 0.0 < tau < math.inf:
        raise ValueError(f"--lap_prior_precision takes a positive number or the word marglik, got {v!r}")
    return tau


def check_lap_flags(args):
    """Whether the run is a Laplace probe (--laplace).  The --lap_* flags belong to it; it is a linear head, so the heads in front of
    it in HEADS are refused (check_head); an evaluation needs the data to fit on or a saved fit, and not both; a saved fit
    belongs to a head that no longer trains."""
    if not check_head(LAP, args):
        return False
    lap_prior_precision(args)
    if hasattr(args, "lap_data_path") and hasattr(args, "lap_state"):
        raise ValueError("--lap_data_path fits the Laplace factors and --lap_state loads them: give one")
    if args.eval and not (hasattr(args, "lap_data_path") or hasattr(args, "lap_state")):
        raise ValueError("--eval --laplace needs --lap_data_path DIR (the labelled images to fit on) or --lap_state FILE (a saved fit)")
    if hasattr(args, "lap_state") and not args.eval:
        raise ValueError("--lap_state is the fit of a finished head: give --eval")
    return True


def laplace_lines(fit, stats):
    """The two lines in front of `* Acc@1`, from fit_laplace's result (with its `source`) and the evaluation's stats."""
    how = fit["source"] + (", grid edge" if fit["on_grid_edge"] else "")
    return ["* Laplace prior precision {:g} ({}) log-marglik {:.5f} NLL {:.5f} on {} images".format(
                fit["prior_precision"], how, fit["log_marglik"], fit["nll"] / max(fit["n"], 1), fit["n"]),
            "* Laplace variance mean {:.6f}".format(stats["lap_var_mean"])]


def laplace_log_entries(fit, stats):
    """What log.txt gains: the prior precision in use, its log marginal likelihood and the mean lap_var of the evaluation."""
    return {"test_lap_prior_precision": fit["prior_precision"], "test_lap_log_marglik": fit["log_marglik"],
            "test_lap_var_mean": stats["lap_var_mean"]}


MAHA_FLAGS = ("maha_data_path", "maha_shrinkage", "maha_state")


def check_maha_flags(args):
    """How the run gets its Mahalanobis density: "fit" (--maha_data_path), "state" (--maha_state) or None.  The three --maha_* flags
    belong to --eval, the two sources are exclusive, --maha_shrinkage needs one of them and is positive and finite."""
    if not any(hasattr(args, k) for k in MAHA_FLAGS):
        return None
    if not args.eval:
        raise ValueError("--maha_data_path / --maha_shrinkage / --maha_state belong to an evaluation: give --eval")
    if hasattr(args, "maha_data_path") and hasattr(args, "maha_state"):
        raise ValueError("--maha_data_path fits the Mahalanobis density and --maha_state loads it: give one")
    if hasattr(args, "maha_shrinkage") and not 0.0 < args.maha_shrinkage < math.inf:
        raise ValueError(f"--maha_shrinkage must be positive and finite, got {args.maha_shrinkage}")
    if hasattr(args, "maha_data_path"):
        return "fit"
    if hasattr(args, "maha_state"):
        return "state"
    raise ValueError("--maha_shrinkage steers the fit of --maha_data_path DIR or --maha_state FILE: give one")


KNN_FLAGS = ("knn_data_path", "knn_state", "knn_k", "knn_temperature")


def check_knn_flags(args):
    """How the run gets its neighbour bank: "fit" (--knn_data_path), "state" (--knn_state) or None.  The four --knn_* flags belong to
    --eval, the two sources are exclusive, --knn_k / --knn_temperature need one of them; k lies in [1, 256] and the temperature is
    positive and finite."""
    if not any(hasattr(args, k) for k in KNN_FLAGS):
        return None
    if not args.eval:
        raise ValueError("--knn_data_path / --knn_state / --knn_k / --knn_temperature belong to an evaluation: give --eval")
    if hasattr(args, "knn_data_path") and hasattr(args, "knn_state"):
        raise ValueError("--knn_data_path fits the neighbour bank and --knn_state loads it: give one")
    if hasattr(args, "knn_k") and not 1 <= args.knn_k <= 256:
        raise ValueError(f"--knn_k must lie in [1, 256], got {args.knn_k}")
    if hasattr(args, "knn_temperature") and not 0.0 < args.knn_temperature < math.inf:
        raise ValueError(f"--knn_temperature must be positive and finite, got {args.knn_temperature}")
    if hasattr(args, "knn_data_path"):
        return "fit"
    if hasattr(args, "knn_state"):
        return "state"
    raise ValueError("--knn_k / --knn_temperature steer the bank of --knn_data_path DIR or --knn_state FILE: give one")


def knn_lines(fit, stats):
    """The two lines in front of `* Acc@1`, from fit_neighbours' (or load_neighbour_state's) result and the evaluation's stats."""
    return ["* kNN bank of {n} images ({skipped} skipped), {classes} classes, k {k}, temperature {temperature:g}".format(**fit),
            "* kNN Acc@1 {knn_acc1:.3f} mean {knn_mean:.5f}".format(**stats)]


def knn_log_entries(fit, stats):
    """What log.txt gains: the weighted k-NN accuracy, the mean knn of the evaluation set and the k in use."""
    return {"test_knn_acc1": stats["knn_acc1"], "test_knn_mean": stats["knn_mean"], "test_knn_k": fit["k"]}


VIM_FLAGS = ("vim_data_path", "vim_dim", "vim_state")


def check_vim_flags(args):
    """How the run gets its ViM fit: "fit" (--vim_data_path), "state" (--vim_state) or None.  The three --vim_* flags belong to --eval,
    the two sources are exclusive, --vim_dim (at least 1) steers a fit on --vim_data_path.  ViM needs a head whose logits are affine
    in the feature: --gp_layer, --het_layer and --ensembles --ens_combine probs are refused."""
    if not any(hasattr(args, k) for k in VIM_FLAGS):
        return None
    if not args.eval:
        raise ValueError("--vim_data_path / --vim_dim / --vim_state belong to an evaluation: give --eval")
    if hasattr(args, "vim_data_path") and hasattr(args, "vim_state"):
        raise ValueError("--vim_data_path fits ViM and --vim_state loads it: give one")
    if hasattr(args, "vim_dim") and args.vim_dim < 1:
        raise ValueError(f"--vim_dim must lie in [1, C - 1], got {args.vim_dim}")
    if not all(head.affine(args) for head in HEADS if getattr(args, head.switch or "", False)):
        raise ValueError("--vim_* need logits that are affine in the feature: not with --gp_layer, --het_layer or --ens_combine probs")
    if hasattr(args, "vim_state"):
        if hasattr(args, "vim_dim"):
            raise ValueError("--vim_dim steers the fit of --vim_data_path DIR: a saved fit keeps its dimension (alpha needs the rows)")
        return "state"
    if hasattr(args, "vim_data_path"):
        return "fit"
    raise ValueError("--vim_dim steers the fit of --vim_data_path DIR: give it")


def vim_lines(fit, stats, embed_dim):
    """The two lines in front of `* Acc@1`, from fit_vim's (or load_vim_state's) result and the evaluation's stats."""
    return ["* ViM fit on {n} images ({skipped} skipped), dim {dim} of {}, alpha {alpha:.5f}, explained {explained:.5f}".format(embed_dim, **fit),
            "* ViM Acc@1 {vim_acc1:.3f} mean {vim_mean:.5f}".format(**stats)]


def vim_log_entries(fit, stats):
    """What log.txt gains: the snapshot head's accuracy, the mean vim of the evaluation set, the dimension and alpha in use."""
    return {"test_vim_acc1": stats["vim_acc1"], "test_vim_mean": stats["vim_mean"], "test_vim_dim": fit["dim"], "test_vim_alpha": fit["alpha"]}


def maha_lines(fit, stats):
    """The two lines in front of `* Acc@1`, from fit_density's result and the evaluation's stats."""
    return ["* Mahalanobis fit on {n} images ({skipped} skipped), {classes} classes ({empty_classes} empty), shrinkage {shrinkage:g}, "
            "log-det {logdet:.5f} background {logdet0:.5f}".format(**fit),
            "* Mahalanobis Acc@1 {maha_acc1:.3f} mean {maha_mean:.5f}".format(**stats)]


def maha_log_entries(fit, stats):
    """What log.txt gains: the nearest-class-mean accuracy, the mean maha of the evaluation set and the shrinkage in use."""
    return {"test_maha_acc1": stats["maha_acc1"], "test_maha_mean": stats["maha_mean"], "test_maha_shrinkage": fit["shrinkage"]}


def conformal_lines(fit, conformal):
    """One line per alpha, from fit_conformal's result and evaluate_conformal's stats["conformal"]."""
    return ["* Conformal {} alpha {:g} qhat {:.5f} coverage {coverage:.5f} size {size:.3f} empty {empty:.5f} singleton {singleton:.5f} "
            "SSCV {sscv:.5f} worst-class {worst_class:.5f} on {} calibration images".format(fit["score"], a, q, fit["n"], **conformal[a])
            for a, q in zip(fit["alpha"], fit["qhat"])]


def conformal_log_entries(fit, conformal):
    """What log.txt gains: the per-alpha lists in --cp_alpha order and the number of calibration images used."""
    rows = [conformal[a] for a in fit["alpha"]]
    out = {"test_cp_alpha": list(fit["alpha"]), "test_cp_qhat": list(fit["qhat"])}
    out.update({f"test_cp_{key}": [r[key] for r in rows] for key in ("coverage", "size", "empty", "singleton", "sscv", "worst_class")})
    out["test_cp_n_cal"] = fit["n"]
    return out


def detection_lines(det):
    """One line per column and question, from stats["detection"]."""
    lines = ["* Detect misclassification {} AUROC {AUROC:.5f} AUPR {AUPR:.5f} FPR95 {FPR95:.5f} AURC {AURC:.5f}".format(c, **det["misclassification"][c])
             for c in det["columns"]]
    if "ood" in det:
        lines += ["* Detect OOD {} AUROC {AUROC:.5f} AUPR {AUPR:.5f} FPR95 {FPR95:.5f}".format(c, **det["ood"][c]) for c in det["columns"]]
    return lines


def detection_log_entries(det):
    """What log.txt gains: test_mis_<column>_<metric> and, with OOD images, test_ood_<column>_<metric>."""
    out = {f"test_mis_{c}_{k}": v for c in det["columns"] for k, v in det["misclassification"][c].items()}
    if "ood" in det:
        out.update({f"test_ood_{c}_{k}": v for c in det["columns"] for k, v in det["ood"][c].items()})
    return out


def perturbation_files(args):
    """[(name, path)] of the perturbations to evaluate: --perturbations as given, else every *.npy of --perturbation_path, sorted."""
    root = args.perturbation_path
    names = getattr(args, "perturbations", None)
    if names is None:
        names = sorted(f[:-4] for f in os.listdir(root) if f.endswith(".npy"))
    if not names:
        raise FileNotFoundError(f"no *.npy under --perturbation_path {root}")
    return [(n, os.path.join(root, n + ".npy")) for n in names]


def check_perturbation_flags(args):
    """Whether the run evaluates perturbation sequences: --perturbation_path, which belongs to --eval, as --perturbations does to it."""
    if (hasattr(args, "perturbation_path") or hasattr(args, "perturbations")) and not (args.eval and hasattr(args, "perturbation_path")):
        raise ValueError("--perturbation_path / --perturbations belong to an evaluation: give --eval and --perturbation_path DIR")
    return hasattr(args, "perturbation_path")


def evaluate_perturbations(args, probe, device, logit_kw=None):
    """The reference's p_evaluate() (uncertainty_evaluations.py:614-658) over perturbation_files(args), V = max(1, batch_size // F)
    sequences per forward (`logit_kw`: the head's own keywords of its logits); prints its lines and returns {name: evaluate_stability's
    result}."""
    aug = BEiTAugment(args.input_size, 1, "bicubic", args.imagenet_default_mean_and_std)
    print("Perturbed dataset evaluation :")
    results, flip_list = {}, []
    for name, path in perturbation_files(args):
        print("Perturbation : " + name)
        ds = PerturbationSequences(path, aug)
        loader = torch.utils.data.DataLoader(ds, batch_size=max(1, args.batch_size // ds.frames), shuffle=False, drop_last=False,
                                             num_workers=args.num_workers, pin_memory=True, collate_fn=collate_sequences)
        r = probe.evaluate_stability(DevicePrefetcher(loader, device), ds.frames, "noise" in name, n_sequences=len(ds), **(logit_kw or {}))
        results[name] = r
        flip_list.append(r["flip_prob"])
        print("\n" + name, "Flipping Prob")
        print(r["flip_prob"])
        print("Top5 Distance\t{:.5f}".format(r["top5_dist"]))
        print("Zipf Distance\t{:.5f}".format(r["zipf_dist"]))
        if r["nan_sequences"]:
            print("%d of %d sequences hold a NaN logit and are left out" % (r["nan_sequences"], r["n_sequences"]))
        if args.output_dir:
            append_log(args.output_dir, {f"test_flip_{name}": r["flip_prob"], f"test_top5_{name}": r["top5_dist"], f"test_zipf_{name}": r["zipf_dist"]})
    print(flip_list)
    print("\nMean Flipping Prob\t{:.5f}".format(np.mean(flip_list)))
    return results


CORRUPTION_FLAGS = ("corruptions", "corruption_severities", "corruption_seed", "corruption_cache_images", "corruption_path")
# uncertainty_evaluations.py:846: the order of the reference's sweep over a pre-made tree
REFERENCE_DISTORTIONS = ("gaussian_noise", "shot_noise", "impulse_noise", "defocus_blur", "glass_blur", "motion_blur", "zoom_blur", "snow",
                         "frost", "brightness", "contrast", "elastic_transform", "pixelate", "jpeg_compression", "speckle_noise")


def check_corruption_flags(args):
    """Where the corruption sweep takes its images from: "device" (--corruptions: generated from --eval_data_path), "path"
    (--corruption_path: a pre-made tree) or None.  All --corruption* flags belong to --eval, the two sources are exclusive,
    --corruptions needs --eval_data_path, and the seed and the cache belong to the generated sets."""
    given = [k for k in CORRUPTION_FLAGS if hasattr(args, k)]
    if not given:
        return None
    if not args.eval:
        raise ValueError("--corruptions / --corruption_* belong to an evaluation: give --eval")
    if hasattr(args, "corruptions") and hasattr(args, "corruption_path"):
        raise ValueError("--corruptions generates the corrupted sets and --corruption_path reads them: give one")
    for s in getattr(args, "corruption_severities", ()):
        if not 1 <= s <= 5:
            raise ValueError(f"--corruption_severities takes severities 1 .. 5, got {s}")
    if len(set(getattr(args, "corruption_severities", ()))) != len(getattr(args, "corruption_severities", ())):
        raise ValueError("--corruption_severities names a severity twice")
    if hasattr(args, "corruption_path"):
        if hasattr(args, "corruption_seed") or hasattr(args, "corruption_cache_images"):
            raise ValueError("--corruption_seed / --corruption_cache_images steer the sets that --corruptions generates: not with --corruption_path")
        return "path"
    if not hasattr(args, "corruptions"):
        raise ValueError("--corruption_severities / --corruption_seed / --corruption_cache_images steer a sweep: give --corruptions NAME ... "
                         "or --corruption_path DIR")
    if not args.eval_data_path:
        raise ValueError("--corruptions corrupts the clean evaluation images: give --eval_data_path DIR")
    if getattr(args, "corruption_cache_images", 0) < 0:
        raise ValueError(f"--corruption_cache_images must be >= 0, got {args.corruption_cache_images}")
    corruption_names(args)
    return "device"


def corruption_names(args):
    """--corruptions as a list of kinds in the order given (`all`: the nine of CORRUPTIONS in their order; `full`: those followed by the
    four of CORRUPTIONS_EXT); an unknown or repeated name is refused."""
    names = list(args.corruptions)
    if names == ["all"]:
        return list(CORRUPTIONS)
    if names == ["full"]:
        return list(CORRUPTIONS + CORRUPTIONS_EXT)
    for n in names:
        if n not in CORRUPTIONS + CORRUPTIONS_EXT:
            raise ValueError(f"--corruptions: unknown corruption {n!r}; one of {', '.join(CORRUPTIONS + CORRUPTIONS_EXT)}, or `all` or `full` alone")
    if len(set(names)) != len(names):
        raise ValueError("--corruptions names a corruption twice")
    return names


def corruption_severities(args):
    return list(getattr(args, "corruption_severities", (1, 2, 3, 4, 5)))


def corruption_folders(args):
    """[(distortion, [(severity, folder)])] of --corruption_path: the reference's DISTORTIONS that are there, in its order, then the other
    sub-folders sorted.  A severity folder that is missing is an error that names it."""
    root = args.corruption_path
    have = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
    if not have:
        raise FileNotFoundError(f"no distortion folders under --corruption_path {root}")
    names = [d for d in REFERENCE_DISTORTIONS if d in have] + [d for d in have if d not in REFERENCE_DISTORTIONS]
    out = []
    for name in names:
        sets = []
        for s in corruption_severities(args):
            folder = os.path.join(root, name, str(s))
            if not os.path.isdir(folder):
                raise FileNotFoundError(f"--corruption_path: severity folder {folder} is missing")
            sets.append((s, folder))
        out.append((name, sets))
    return out


def corruption_set_line(stats):
    """uncertainty_evaluations.py:384-386, the trailing blank included."""
    return "* Acc@1 {:.4f} CE {:.4f} ".format(stats["acc1"], (100 - stats["acc1"]) / 100)


def corruption_set_lines(stats):
    """The reference's line of one set, then what its stats hold beyond accuracy: the calibration line, the head's variance mean, the
    misclassification-detection lines."""
    lines = [corruption_set_line(stats)]
    if "ECE" in stats:
        lines.append(calibration_line(stats))
    if "set_calibration" in stats:
        lines.append(set_calibration_line(stats["set_calibration"]))
    lines += [fmt(stats) for key, fmt in VAR_MEAN_LINES if key in stats]
    if "detection" in stats:
        lines += detection_lines(stats["detection"])
    return lines


def corruption_log_entries(name, severity, stats):
    """The set's line of log.txt: test_c_<name>_<severity>_<key>."""
    out = {"acc1": stats["acc1"], "acc5": stats["acc5"], "loss": stats["loss"], "ce": (100 - stats["acc1"]) / 100}
    out.update({k: stats[k] for k in CALIB_KEYS if k in stats})
    out.update({k: stats[k] for k, _ in VAR_MEAN_LINES if k in stats})
    if "set_calibration" in stats:
        out.update(set_calibration_log_entries(stats["set_calibration"], prefix="set_"))
    if "detection" in stats:
        out.update({k[len("test_"):]: v for k, v in detection_log_entries(stats["detection"]).items()})
    return {f"test_c_{name}_{severity}_{k}": v for k, v in out.items()}


def corruption_summary(results, clean_stats):
    """{"mce", "acc", "severities", "acc1", "ce", "rel_ce"[, "ECE", "NLL"]} of results = {(name, severity): stats}: the reference's
    closing figures (the mean CE and the mean accuracy over all sets) and, per severity in ascending order, the means over the
    corruptions evaluated at it; rel_ce is the CE minus the clean run's."""
    ce = lambda s: (100 - s["acc1"]) / 100      # noqa: E731
    sets = list(results.values())
    out = {"mce": float(np.mean([ce(s) for s in sets])), "acc": float(np.mean([s["acc1"] for s in sets]))}
    sevs = sorted({sev for _, sev in results})
    rows = {sev: [s for (_, v), s in results.items() if v == sev] for sev in sevs}
    out["severities"] = sevs
    out["acc1"] = [float(np.mean([s["acc1"] for s in rows[v]])) for v in sevs]
    out["ce"] = [float(np.mean([ce(s) for s in rows[v]])) for v in sevs]
    out["rel_ce"] = [c - ce(clean_stats) for c in out["ce"]]
    for key in ("ECE", "NLL"):
        if all(key in s for s in sets):
            out[key] = [float(np.mean([s[key] for s in rows[v]])) for v in sevs]
    if all("set_calibration" in s for s in sets):
        for key in SCAL_SUMMARY_KEYS:
            out["set_" + key] = [float(np.mean([s["set_calibration"][key] for s in rows[v]])) for v in sevs]
    return out


def corruption_summary_lines(summary):
    """The reference's closing line (uncertainty_evaluations.py:391), then one line per severity (Ovadia et al. 2019's table)."""
    lines = ["mCE (unnormalized) (%): {:.4f}, acc :{:.4f}".format(summary["mce"], summary["acc"])]
    for i, sev in enumerate(summary["severities"]):
        line = "* Severity {} Acc@1 {:.4f} CE {:.4f} rel-CE {:.4f}".format(sev, summary["acc1"][i], summary["ce"][i], summary["rel_ce"][i])
        if "ECE" in summary:
            line += " ECE {:.5f} NLL {:.5f}".format(summary["ECE"][i], summary["NLL"][i])
        if "set_ECE" in summary:
            line += " set-ECE {:.5f} Brier {:.5f}".format(summary["set_ECE"][i], summary["set_Brier"][i])
        lines.append(line)
    return lines


def corruption_summary_log(summary):
    out = {"test_c_mce": summary["mce"], "test_c_acc": summary["acc"], "test_c_severity_levels": summary["severities"]}
    out.update({f"test_c_severity_{k}": summary[k] for k in ("acc1", "ce", "rel_ce", "ECE", "NLL", "set_ECE", "set_NLL", "set_Brier") if k in summary})
    return out


def evaluate_corruptions(args, probe, device, clean_stats, eval_kw=None):
    """The reference's c_evaluate() (uncertainty_evaluations.py:355-391) behind the main evaluation: per distortion and severity one
    probe.evaluate with the run's own switches (`eval_kw`: calibration, detection, temperature and the head's), the reference's lines
    with the additions of corruption_set_lines, its closing mCE line and the per-severity summary.  With --corruptions the sets are
    generated on the device from the clean evaluation folder (uncertainty_vit_amd/corruptions.py): the first set reads and packs the
    folder into a CleanCache, the others replay it; a folder over --corruption_cache_images is read again per set.  With
    --corruption_path every DIR/<distortion>/<severity> is read with the evaluation pipeline.  Returns {"sets": {(name, severity):
    stats}, "summary": corruption_summary's}."""
    eval_kw = dict(eval_kw or {})
    eval_kw.pop("ood_loader", None)          # the sets are compared with themselves: misclassification detection only
    if hasattr(args, "corruption_path"):
        # the loaders first: their `Eval data = ...` lines stay out of the reference's block
        plan = [(name, [(s, build_loader(args, probe.encoder, folder, 1, train=False)[0]) for s, folder in sets])
                for name, sets in corruption_folders(args)]
        make = lambda name, s, loader: DevicePrefetcher(loader, device)      # noqa: E731
    else:
        aug = BEiTAugment(args.input_size, 1, "bicubic", args.imagenet_default_mean_and_std)
        loader, _ = build_loader(args, probe.encoder, args.eval_data_path, 1, train=False)
        cache = CleanCache(getattr(args, "corruption_cache_images", DEFAULT_CACHE_IMAGES), args.batch_size)
        seed = getattr(args, "corruption_seed", 0)
        plan = [(name, [(s, None) for s in corruption_severities(args)]) for name in corruption_names(args)]

        def make(name, s, _):
            if cache.ready:
                return CorruptedSet(cache, name, s, seed, aug.mean, aug.std)
            return CorruptedSet(DevicePrefetcher(loader, device), name, s, seed, aug.mean, aug.std, cache=None if cache.overflowed else cache)
    print("Corrupted dataset evaluation :")
    results = {}
    for name, sets in plan:
        print("Distortion : " + name)
        for s, loader_c in sets:
            stats = probe.evaluate(make(name, s, loader_c), **eval_kw)
            results[(name, s)] = stats
            print("\n".join(corruption_set_lines(stats)))
            if args.output_dir:
                append_log(args.output_dir, corruption_log_entries(name, s, stats))
    summary = corruption_summary(results, clean_stats)
    print("\n".join(corruption_summary_lines(summary)))
    if args.output_dir:
        append_log(args.output_dir, corruption_summary_log(summary))
    return {"sets": results, "summary": summary}


def encoder_kwargs(checkpoint):
    """Constructor options of the encoder a run_cyclical.py checkpoint was trained with (utils.save_model keeps its args)."""
    a = checkpoint.get("args") if isinstance(checkpoint, dict) else None
    return dict(use_shared_rel_pos_bias=getattr(a, "rel_pos_bias", True), use_abs_pos_emb=getattr(a, "abs_pos_emb", False),
                init_values=getattr(a, "layer_scale_init_value", 0.1))


def build_loader(args, encoder, root, aug_level, train):
    if args.data_set not in FOLDER_DATA_SETS:
        raise NotImplementedError(f"--data_set {args.data_set} needs torchvision's archive format; use an image folder")
    aug = BEiTAugment(args.input_size, aug_level, "bicubic", args.imagenet_default_mean_and_std)
    ds = ImageFolderPretrain(root, aug, encoder.patch_embed.patch_shape, 0)      # no masked patches: the probe's forward takes no mask
    print(("Train" if train else "Eval") + " data = %s, %d images, %d classes" % (aug, len(ds), len(ds.classes)))
    return torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=train, drop_last=train, num_workers=args.num_workers,
                                       pin_memory=True, collate_fn=collate_packed), ds


def save_probe(args, probe, epoch):
    path = Path(args.output_dir) / f"probe-{epoch}.pth"
    torch.save({"model": {k: v.cpu() for k, v in probe.state_dict().items()}, "optimizer": probe.optimizer_state_dict(), "epoch": epoch,
                "args": vars(args)}, path)
    return path


@dataclass(frozen=True)
class Head:
    build: callable                               # (args, encoder) -> the probe
    switch: str = None                            # the args attribute that selects it; None: a fallback, taken when no switch is given
    two_stream: bool = False                      # a fallback: for which kind of encoder
    flags: tuple = ()                             # the options that belong to it
    orphan: str = ""                              # the refusal of an option without the switch
    beside: str = ""                              # the refusal beside a head earlier in HEADS; {}: the switches in front of its own
    check: callable = None                        # (args): what it validates beyond check_head
    encoder_kw: callable = lambda args: {}        # the constructor options it asks of the encoder (asked of every head: {} where its flags are absent)
    check_encoder: callable = None                # (args, encoder): runs for every head once the encoder is built
    eval_kw: callable = lambda args: {}           # its own keywords of probe.evaluate
    logit_kw: callable = lambda args: {}          # those of every call that forms logits: temperature fit, conformal sets, perturbations
    affine: callable = lambda args: True          # whether its logits are affine in the feature
    extend: callable = None                       # (args, probe, ctx, stats): adds to an evaluation's stats
    lines: callable = lambda stats, dims: []      # its lines behind `* Acc@1`
    log: callable = lambda stats: {}              # its entries of log.txt
    var_mean: tuple = None                        # (stats key, line) of the variance mean that a corrupted set reports
    epoch_start: callable = None                  # (probe): in front of a training epoch


def check_head(head, args):
    """Whether `head` is selected.  Its options are refused without its switch, and so is the head beside one that stands earlier in
    HEADS: the later head speaks, and names every switch in front of its own."""
    if not getattr(args, head.switch, False):
        if any(hasattr(args, k) for k in head.flags):
            raise ValueError(head.orphan)
        return False
    earlier = [h.switch for h in HEADS[:HEADS.index(head)] if h.switch]
    if any(getattr(args, k, False) for k in earlier):
        raise ValueError(head.beside.format(" / ".join("--" + k for k in earlier)))
    return True


def check_ens_heads(args):
    """check_head, and --ens_heads: it assembles an ensemble for an evaluation, in place of --resume, and sets the member count."""
    heads = getattr(args, "ens_heads", None)
    if check_head(ENS, args) and heads is not None:
        if not args.eval:
            raise ValueError("--ens_heads assembles an ensemble for an evaluation: give --eval")
        if args.resume:
            raise ValueError("--ens_heads and --resume both name the heads: give one")
        if hasattr(args, "ens_members") and args.ens_members != len(heads):
            raise ValueError(f"--ens_members {args.ens_members} but --ens_heads names {len(heads)} files")


def build_ens(args, encoder):
    kw = dict(smoothing=args.smoothing, **given(args, "ens_", ("combine", "bagging", "seed")))
    if not hasattr(args, "ens_heads"):
        return ens_probe.EnsembleProbe(encoder, args.nb_classes, members=ens_member_count(args), **kw)
    heads = [torch.load(path, map_location="cpu", weights_only=False)["model"] for path in args.ens_heads]
    probe = ens_probe.EnsembleProbe.from_heads(encoder, heads, **kw)
    if probe.num_classes != args.nb_classes:
        raise ValueError(f"--ens_heads hold {probe.num_classes} classes, --nb_classes is {args.nb_classes}")
    print("Ensemble of %d heads: %s" % (probe.members, list(args.ens_heads)))
    return probe


GP = Head(lambda args, enc: gp_probe.GPProbe(enc, args.nb_classes, smoothing=args.smoothing,
                                             **given(args, "gp_", ("num_inducing", "kernel_scale", "cov_momentum", "cov_ridge_penalty"))),
          switch="gp_layer", flags=GP_FLAGS, orphan="--gp_* options belong to the GP head: give --gp_layer",
          eval_kw=lambda args: {"variance": True, **given(args, "gp_", ("mean_field",))}, logit_kw=lambda args: given(args, "gp_", ("mean_field",)),
          affine=lambda args: False, lines=lambda stats, dims: [gp_variance_line(stats)], log=lambda stats: {"test_gp_var_mean": stats["gp_var_mean"]},
          var_mean=("gp_var_mean", gp_variance_line),      # the exact sum counts the data once: it starts again with every epoch
          epoch_start=lambda probe: probe.reset_cov() if probe.cov_momentum <= 0 else None)
HET = Head(lambda args, enc: het_probe.HetProbe(enc, args.nb_classes, smoothing=args.smoothing,
                                                **given(args, "het_", ("num_factors", "temperature", "train_mc_samples", "test_mc_samples", "seed"))),
           switch="het_layer", flags=HET_FLAGS, orphan="--het_* options belong to the heteroscedastic head: give --het_layer",
           beside="--het_layer and --gp_layer are two heads: give one", eval_kw=lambda args: {"variance": True}, affine=lambda args: False,
           lines=lambda stats, dims: [het_variance_line(stats)], log=lambda stats: {"test_het_var_mean": stats["het_var_mean"]},
           var_mean=("het_var_mean", het_variance_line))
ENS = Head(build_ens, switch="ensembles", flags=ENS_FLAGS, orphan="--ens_* options belong to the ensemble: give --ensembles",
           beside="--ensembles is an ensemble of linear heads: give it without {}", check=check_ens_heads,
           eval_kw=lambda args: {"members": True, "uncertainty": True}, affine=lambda args: getattr(args, "ens_combine", "logits") != "probs",
           lines=lambda stats, dims: ens_lines(stats), log=ens_log_entries)
# its fit, and with it its lines and its part of log.txt, is the family of the same name; variance=True is an evaluation's alone
LAP = Head(lambda args, enc: lap_probe.LaplaceProbe(enc, args.nb_classes, smoothing=args.smoothing), switch="laplace", flags=LAP_FLAGS,
           orphan="--lap_* options belong to the Laplace probe: give --laplace", eval_kw=lambda args: {"variance": True} if args.eval else {},
           beside="--laplace is a post-hoc fit of the linear head: give it without {}",
           var_mean=("lap_var_mean", lambda stats: "* Laplace variance mean {lap_var_mean:.6f}".format(**stats)))
MCD = Head(lambda args, enc: mcd_probe.MCDropoutProbe(enc, args.nb_classes, smoothing=args.smoothing, passes=args.mc_dropout_forwards,
                                                      **given(args, "mc_dropout_", ("layers",)), **given(args, "mc_", ("combine", "seed"))),
           switch="mc_dropout_forwards", flags=MCD_FLAGS + ("attn_drop_rate",),      # the probe's forward is dropout-free without it
           orphan="--mc_* options and --attn_drop_rate belong to MC-dropout: give --mc_dropout_forwards T", check=check_mcd_flags,
           beside="--mc_dropout_forwards samples the linear head: give it without {}", eval_kw=lambda args: {"uncertainty": True},
           encoder_kw=lambda args: given(args, "", ("attn_drop_rate",)),             # check_head has refused the rate without the switch
           lines=lambda stats, dims: mcd_lines(stats, dims.depth, dims.attn_drop_rate), log=mcd_log_entries)
LW = Head(lambda args, enc: lw_probe.LayerWeightedProbe(enc, args.nb_classes, smoothing=args.smoothing,
                                                        **given(args, "", ("use_cls", "layernorm_before_combine"))),
          switch="learn_layer_weights", flags=("layernorm_before_combine", "use_cls"),
          orphan="--layernorm_before_combine / --use_cls belong to the layer-weighted probe: give --learn_layer_weights "
                 "(--use_cls alone needs a trained final norm, which is not built)",
          beside="--learn_layer_weights mixes the features of the linear head: give it without {}",
          check=lambda args: check_lw_flags(args) and args.target_layer != -1 and print(
              "--learn_layer_weights supersedes --target_layer %d: the encoder keeps every block" % args.target_layer),      # run_class_finetuning.py:520
          encoder_kw=lambda args: {"target_layer": -1} if getattr(args, "learn_layer_weights", False) else {},
          extend=lambda args, probe, ctx, stats: stats.update(layer_weights=probe.layer_weights().cpu().tolist()),
          lines=lambda stats, dims: [layer_weights_line(stats["layer_weights"])], log=lambda stats: {"test_layer_weights": stats["layer_weights"]})
# check_dist_flags runs for every head: it refuses the --dist_* flags of a base model, and a factor > 0 beside ViM, which needs affine logits
DIST = Head(lambda args, enc: dist_probe.DistProbe(enc, args.nb_classes, smoothing=args.smoothing, **given(args, "dist_", ("mean_field", "var_scale"))),
            two_stream=True, check_encoder=lambda args, encoder: check_dist_flags(args, encoder._two_stream), eval_kw=lambda args: {"variance": True},
            lines=lambda stats, dims: [dist_variance_line(stats)], var_mean=("dist_var_mean", dist_variance_line),
            log=lambda stats: {"test_dist_var_mean": stats["dist_var_mean"], "test_dist_trace_mean": stats["dist_trace_mean"]})
LINEAR = Head(lambda args, enc: linear_probe.LinearProbe(enc, args.nb_classes, smoothing=args.smoothing))
HEADS = (GP, HET, ENS, LAP, MCD, LW, DIST, LINEAR)      # the order is the precedence, and who speaks when two switches are given
VAR_MEAN_LINES = tuple(h.var_mean for h in HEADS if h.var_mean)


@dataclass(frozen=True)
class Family:
    name: str
    check: callable                               # its check_*_flags: None or False leaves the family out of the run, anything else is its mode
    implies: tuple = ()                           # the families that a mode of this one switches on
    prepare: callable = None                      # (args, probe, ctx) -> the fit, made or loaded in front of the evaluation; without: the mode
    per_epoch: bool = False                       # the fit is of the head as it stands: a training run repeats it behind every epoch's steps
    eval_kw: callable = None                      # (args, fit) -> its keywords of probe.evaluate
    returned_as: str = None                       # the key of the fit in an --eval run's stats
    extend: callable = None                       # (args, probe, ctx, stats): adds to an evaluation's stats
    front: callable = None                        # (fit, stats, dims) -> its lines in front of `* Acc@1`
    behind: callable = None                       # (fit, stats, dims) -> its lines behind it, after the head's
    log: callable = None                          # (fit, stats) -> its entries of log.txt
    log_leads: bool = False                       # ... in front of the head's, where the four calibration keys have always stood
    after: callable = None                        # (args, probe, ctx, stats): follows an --eval run's report


def fit_or_load(args, ctx, prefix, names, fit, save, file, load, what):
    """The two sources of a saved fit, `own` being the --<prefix>_<name> given: --<prefix>_data_path DIR gives fit(loader of DIR, **own), with
    --output_dir saved as `file` (save(fit): what goes into it); --<prefix>_state FILE gives load(what FILE holds, overridden by own)."""
    own = given(args, prefix + "_", names)
    if hasattr(args, prefix + "_data_path"):
        out = fit(ctx.loader(getattr(args, prefix + "_data_path")), **own)
        if args.output_dir:
            torch.save(save(out), os.path.join(args.output_dir, file))
        return out
    if hasattr(args, prefix + "_state"):
        out = load({**torch.load(getattr(args, prefix + "_state"), map_location="cpu", weights_only=False), **own})
        print("Load %s %s" % (what, getattr(args, prefix + "_state")))
        return out


def prepare_laplace(args, probe, ctx):
    """The fit on --lap_data_path for the head as it stands, or the one of --lap_state, under --lap_prior_precision when it is given."""
    prior = lap_prior_precision(args)
    source = "marglik" if prior == "marglik" else "given"

    def load(saved):
        out = {**probe.load_laplace_state(saved), "source": saved.get("source", "given"), "on_grid_edge": bool(saved.get("on_grid_edge", False))}
        return out if prior is None else {**probe.set_prior_precision(prior), "source": source}

    return fit_or_load(args, ctx, "lap", (), lambda loader: {**probe.fit_laplace(loader, prior_precision=1.0 if prior is None else prior), "source": source},
                       lambda out: {**probe.laplace_state_dict(), "source": out["source"], "on_grid_edge": out["on_grid_edge"]}, "laplace.pth",
                       load, "Laplace state")


def prepare_vim(args, probe, ctx):
    def fit(loader, **own):
        same = hasattr(args, "maha_data_path") and os.path.realpath(args.maha_data_path) == os.path.realpath(args.vim_data_path)
        return probe.fit_vim(loader, moments=probe.density_state_dict() if same else None, **own)      # the density's pass has read this folder

    return fit_or_load(args, ctx, "vim", ("dim",), fit, lambda out: probe.vim_state_dict(), "vim.pth", probe.load_vim_state, "ViM state")


def prepare_conformal(args, probe, ctx):
    raps = getattr(args, "cp_score", "aps") == "raps"
    # what the fit and evaluate_conformal share with probe.evaluate: the post-hoc temperature and the head's own keywords
    ctx.conformal_kw = {**{k: v for k, v in ctx.eval_kw.items() if k == "temperature"}, **ctx.head.logit_kw(args)}
    return probe.fit_conformal(ctx.loader(args.cp_data_path), **given(args, "cp_", ("alpha", "score", "randomized", "seed")),
                               lam=getattr(args, "cp_lambda", 0.01) if raps else 0.0, kreg=getattr(args, "cp_kreg", 5) if raps else 0,
                               **ctx.conformal_kw)


def check_corruption_sets(args):
    mode = check_corruption_flags(args)
    if mode == "path":
        corruption_folders(args)                  # a missing folder stops the run here, not behind the main evaluation
    return mode


# the order of the lines in front of `* Acc@1`, of those behind it, of log.txt's keys and of what follows the report
FAMILIES = (
    Family("calibration", lambda args: getattr(args, "calibration", False), eval_kw=lambda args, fit: {"calibration": True},
           behind=lambda fit, stats, dims: [calibration_line(stats)], log=lambda fit, stats: {f"test_{k}": stats[k] for k in CALIB_KEYS}, log_leads=True),
    Family("set_calibration", check_scal_flags,      # last in FIT_ORDER: the fits' passes over the calibration folders store nothing
           prepare=lambda args, probe, ctx: probe.enable_set_calibration(**ctx.modes["set_calibration"]),
           behind=lambda fit, stats, dims: [set_calibration_line(stats["set_calibration"])],
           log=lambda fit, stats: set_calibration_log_entries(stats["set_calibration"]),
           after=lambda args, probe, ctx, stats: write_reliability(args.output_dir, stats["set_calibration"]) if args.output_dir else None),
    Family("detection", check_detection_flags, eval_kw=lambda args, fit: fit,      # the OOD images go through the evaluation's own forward
           behind=lambda fit, stats, dims: detection_lines(stats["detection"]), log=lambda fit, stats: detection_log_entries(stats["detection"]),
           prepare=lambda args, probe, ctx: {"detection": True, **({"ood_loader": ctx.loader(args.ood_data_path)} if hasattr(args, "ood_data_path") else {})}),
    Family("temperature", check_ts_flags, returned_as="temperature_fit",      # --ts_temperature: no fit, and the figure is the keyword
           prepare=lambda args, probe, ctx: probe.fit_temperature(ctx.loader(args.ts_data_path), **given(args, "ts_", ("tol", "max_iter")),
                                                                  **ctx.head.logit_kw(args)) if hasattr(args, "ts_data_path") else None,
           eval_kw=lambda args, fit: {"temperature": args.ts_temperature if fit is None else True},
           front=lambda fit, stats, dims: [temperature_line(fit)] if fit else [], log=lambda fit, stats: temperature_log_entries(stats, fit)),
    Family("laplace", check_lap_flags, prepare=prepare_laplace, per_epoch=True, returned_as="laplace_fit",
           front=lambda fit, stats, dims: laplace_lines(fit, stats) if fit else [],
           log=lambda fit, stats: laplace_log_entries(fit, stats) if fit else {}),
    Family("maha", check_maha_flags, implies=("detection",), returned_as="density_fit",
           prepare=lambda args, probe, ctx: fit_or_load(args, ctx, "maha", ("shrinkage",), probe.fit_density, lambda out: probe.density_state_dict(),
                                                        "density.pth", probe.load_density_state, "Mahalanobis state"),
           front=lambda fit, stats, dims: maha_lines(fit, stats), log=maha_log_entries),
    Family("knn", check_knn_flags, implies=("detection",), returned_as="neighbour_fit",
           prepare=lambda args, probe, ctx: fit_or_load(args, ctx, "knn", ("k", "temperature"), probe.fit_neighbours, lambda out: probe.neighbour_state_dict(),
                                                        "neighbours.pth", probe.load_neighbour_state, "neighbour bank"),
           front=lambda fit, stats, dims: knn_lines(fit, stats), log=knn_log_entries),
    Family("vim", check_vim_flags, implies=("detection",), prepare=prepare_vim, returned_as="vim_fit",
           front=lambda fit, stats, dims: vim_lines(fit, stats, dims.embed_dim), log=vim_log_entries),
    Family("conformal", check_cp_flags, prepare=prepare_conformal, returned_as="conformal_fit",
           extend=lambda args, probe, ctx, stats: stats.update(conformal=probe.evaluate_conformal(ctx.evaluation(), **ctx.conformal_kw)["conformal"]),
           behind=lambda fit, stats, dims: conformal_lines(fit, stats["conformal"]), log=lambda fit, stats: conformal_log_entries(fit, stats["conformal"])),
    Family("perturbations", check_perturbation_flags,
           after=lambda args, probe, ctx, stats: stats.update(stability=evaluate_perturbations(args, probe, ctx.device, ctx.head.logit_kw(args)))),
    Family("corruptions", check_corruption_sets,
           after=lambda args, probe, ctx, stats: stats.update(corruptions=evaluate_corruptions(args, probe, ctx.device, stats, eval_kw=ctx.eval_kw))),
)
# the order of the fits and of the evaluate keywords: the temperature is fitted on the probit-scaled logits and reported in front of them
FIT_ORDER = ("calibration", "detection", "laplace", "maha", "knn", "vim", "temperature", "conformal", "set_calibration")


def validate(args):
    """Every refusal that needs no checkpoint; {family: mode} of the families the run uses."""
    if args.nb_classes < 1:
        raise ValueError("--nb_classes is required")
    if not args.finetune:
        raise ValueError("--finetune <pre-training checkpoint> is required")
    modes = {f.name: mode for f in FAMILIES for mode in [f.check(args)] if mode is not None and mode is not False}
    for f in FAMILIES:
        modes.update({name: True for name in f.implies if f.name in modes and name not in modes})
    for head in (h for h in HEADS if h.switch):
        head.check(args) if head.check else check_head(head, args)
    build_mixer(args)
    build_augmenter(args)
    return modes


def run_fits(args, probe, ctx, fits, families):
    """prepare() and the evaluate keywords of `families`, in FIT_ORDER: `fits` gains every fit, ctx.eval_kw every keyword."""
    for f in sorted((f for f in families if f.name in FIT_ORDER), key=lambda f: FIT_ORDER.index(f.name)):
        if f.prepare:
            fits[f.name] = f.prepare(args, probe, ctx)
        if f.eval_kw:
            ctx.eval_kw.update(f.eval_kw(args, fits[f.name]))


def report(stats, fits, head, families, dims):
    """What an evaluation reports, from its stats, {family: fit} of the families in use, the head's record and `dims` (depth, attn_drop_rate,
    embed_dim): the lines in front of `* Acc@1`, the lines behind it, log.txt's entries (the three figures first).  No I/O, no device."""
    on = [(f, fits[f.name]) for f in families if f.name in fits]
    front = [line for f, fit in on if f.front for line in f.front(fit, stats, dims)]
    behind = head.lines(stats, dims) + [line for f, fit in on if f.behind for line in f.behind(fit, stats, dims)]
    logs = [(f.log_leads, f.log(fit, stats)) for f, fit in on if f.log]
    entries = {f"test_{k}": stats[k] for k in ("loss", "acc1", "acc5")}
    for part in [log for leads, log in logs if leads] + [head.log(stats)] + [log for leads, log in logs if not leads]:
        entries.update(part)
    return front, behind, entries


def main(args):
    print(args)
    if not torch.cuda.is_available():
        raise RuntimeError("the linear probe runs as HIP kernels: a GPU is required")
    modes = validate(args)
    device = torch.device("cuda")
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    ckpt = torch.load(args.finetune, map_location="cpu", weights_only=False)
    print("Load ckpt from %s" % args.finetune)
    own = {"target_layer": args.target_layer, **{k: v for h in HEADS for k, v in h.encoder_kw(args).items()}}
    encoder = linear_probe.build_probe_encoder(args.model, img_size=args.input_size, **encoder_kwargs(ckpt), **own)
    unused = linear_probe.load_encoder_checkpoint(encoder, ckpt, args.model_key, args.model_prefix)
    print(f"encoder: {encoder.depth} blocks, {len(unused)} checkpoint entries not part of it")
    encoder.to(device)
    for h in (h for h in HEADS if h.check_encoder):
        h.check_encoder(args, encoder)
    # the head whose switch is given; without one, the fallback for the encoder's kind
    head = next(h for h in HEADS if (getattr(args, h.switch, False) if h.switch else h.two_stream == encoder._two_stream))
    probe = head.build(args, encoder)
    print("Trainable weights: %s" % [n for n, p in probe.named_parameters() if p.requires_grad])
    mixer = build_mixer(args)
    if mixer is not None:
        print("Mixup is activated!")                  # run_class_finetuning.py:567; train_loss is the soft-target loss from here on
        probe.enable_mix(mixer)
    augmenter = build_augmenter(args)
    if augmenter is not None:
        print("RandAugment is activated: %s" % augmenter)
        probe.enable_randaug(augmenter)
    start_epoch = 0
    if args.resume:
        st = torch.load(args.resume, map_location="cpu", weights_only=False)
        probe.load_state_dict(st["model"])
        probe.load_optimizer_state_dict(st["optimizer"])
        start_epoch = int(st["epoch"]) + 1
        print("Resume checkpoint %s" % args.resume)
    loader_val, _ = build_loader(args, encoder, args.eval_data_path or args.data_path, 1, train=False)
    ctx = SimpleNamespace(device=device, head=head, modes=modes, eval_kw=head.eval_kw(args), evaluation=lambda: DevicePrefetcher(loader_val, device),
                          loader=lambda root: DevicePrefetcher(build_loader(args, encoder, root, 1, train=False)[0], device))
    families, fits = [f for f in FAMILIES if f.name in modes], dict(modes)
    run_fits(args, probe, ctx, fits, [f for f in families if args.eval or not f.per_epoch])
    dims = SimpleNamespace(depth=encoder.depth, attn_drop_rate=encoder.attn_drop_rate, embed_dim=probe.embed_dim)

    def evaluate():
        stats = probe.evaluate(ctx.evaluation(), **ctx.eval_kw)
        for record in (r for r in [head] + families if r.extend):      # a failure here loses the report of the evaluation that has just run
            record.extend(args, probe, ctx, stats)
        return stats

    if args.eval:
        stats = evaluate()
        stats.update({f.returned_as: fits[f.name] for f in families if f.returned_as and fits[f.name] is not None})
        front, behind, entries = report(stats, fits, head, families, dims)
        print("\n".join(front + [f"* Acc@1 {stats['acc1']:.3f} Acc@5 {stats['acc5']:.3f} loss {stats['loss']:.3f} on {stats['n']} test images"] + behind))
        if len(entries) > 3 and args.output_dir:          # --eval alone writes no line
            append_log(args.output_dir, entries)
        for f in (f for f in families if f.after):
            f.after(args, probe, ctx, stats)
        return stats
    loader_train, _ = build_loader(args, encoder, args.data_path, 3, train=True)
    print("LR = %.8f" % args.lr)
    print("Batch size = %d" % args.batch_size)
    steps_per_epoch = len(loader_train)
    print("Number of training steps per epoch = %d" % steps_per_epoch)
    lr_values = utils.cosine_scheduler(args.lr, args.min_lr, args.epochs, steps_per_epoch, warmup_epochs=args.warmup_epochs)

    def publish(log, loss, gnorm):
        loss, gnorm = loss.item(), gnorm.item()
        if not (math.isfinite(loss) and math.isfinite(gnorm)):
            # engine_for_finetuning.py:101-103.  The step was already enqueued: uvit_op_adamw saw the same values and left the head as
            # it was, and nothing is saved after this point
            print("Loss is {}, stopping training".format(loss))
            sys.exit(1)
        log.update(loss=loss, grad_norm=gnorm)

    stats, t0 = None, time.time()
    for epoch in range(start_epoch, args.epochs):
        log, seen = utils.MetricLogger(delimiter="  "), []
        if head.epoch_start:
            head.epoch_start(probe)
        for i, ((images, _), labels) in enumerate(log.log_every(DevicePrefetcher(loader_train, device), 10, f"Epoch: [{epoch}]")):
            lr = float(lr_values[epoch * steps_per_epoch + i])
            loss, gnorm = probe.train_step(images, labels.to(device, non_blocking=True), lr, args.weight_decay, args.clip_grad)
            seen.append((loss.clone(), gnorm.clone()))          # device scalars: read one step late, never in the step's way
            if len(seen) > 1:
                publish(log, *seen.pop(0))
            log.update(lr=lr)
        for l0, g0 in seen:
            publish(log, l0, g0)
        run_fits(args, probe, ctx, fits, [f for f in families if f.per_epoch])      # of this epoch's head: train_step dropped the one before
        stats = evaluate()
        front, behind, entries = report(stats, fits, head, families, dims)
        print("\n".join(front + [f"* Acc@1 {stats['acc1']:.3f} Acc@5 {stats['acc5']:.3f} loss {stats['loss']:.3f}"] + behind))
        print(f"Epoch {epoch}: loss: {log.loss.global_avg:.4f}  lr: {log.lr.value:.8f}  acc1: {stats['acc1']:.3f}  acc5: {stats['acc5']:.3f}")
        if args.output_dir:
            save_probe(args, probe, epoch)
            append_log(args.output_dir, {"epoch": epoch, "train_loss": log.loss.global_avg, "train_lr": log.lr.value, **entries})
    print("Training time %.0f s" % (time.time() - t0))
    return stats


if __name__ == "__main__":
    opts = get_args()
    if opts.output_dir:
        Path(opts.output_dir).mkdir(parents=True, exist_ok=True)
    main(opts)
