"""main.lua's training driver over the fused engine: `train` (main.lua:12-50), `test` (:52-69) and the epoch loop of
`run` (:138-184) -- the immediate caller of the hot path, S-draw loop included (main.lua:28-40).

    opt = default_opt(hidden=[400, 400]); train_set, test_set = data.getMnist(root)
    Main(opt).run(train_set, test_set, epochs=10)

Per minibatch: resetGradients; prepare (compute_prior + operand packing); S x { sample; run }; update -- every
launch on the device, ONE host synchronisation per minibatch (the loss / accuracy read-back the reference's
`net:run` return values need). Per epoch: the five series of main.lua:169-177 through vbnn_amd.logger, and the run
directory's `parameters/means`, `parameters/vars`, `opt` (the files mainviz.lua:11-15 loads) through
vbnn_amd.t7file with utils.safe_save's keep-the-old-file rule (main.lua:181 saves the whole Lua `net` table, methods
included; Lua byte code cannot be produced here, so the data is what is saved).

opt.prune_schedule = [(epoch, fraction), ...] (off by default; epochs count from 0 over the life of this Main): at the start of
each listed epoch the trainer prunes that fraction of the weights by signal-to-noise (FusedMLP.prune, opt.prune_scope, default
"global") and HOLDS the mask through the training that follows (FusedMLP.hold_pruned) -- prune, retrain, prune again. The masks
are ORed, and prune() ranks the frozen weights by the values they were frozen with, so the held fraction can exceed the listed
one; the series `held fraction` logs the true one, and `lc` is then the kept weights' sum. The reference only counts what
would go (mainviz.lua:20-27).

opt.checkpoint = True (off by default): save() also writes `<network_name>/model` -- the engine's complete state (FusedMLP.save) plus
trainer = {epoch, indices, rng}; opt.network_to_load = <dir> loads `<dir>/model` into the engine and restores the trainer, and the run
continues bit for bit as the uninterrupted one would have (checkpoint.py says why).

opt.calibration_bins = M (0 = off, the default) with opt.predictive and the NLL criterion: the dev pass accumulates ONE
CalibrationResult over its minibatches (FusedMLP.calibration, into=) and logs `dev_ece`, `dev_mce`, `dev_brier`;
opt.selective_coverages = [c, ...] adds `dev_acc@cov<c>`, the accuracy over the fraction c of the dev rows the predictive entropy
ranks most certain (FusedMLP.selective).

opt.ranking = True (off by default) with opt.predictive and the "bce" or "nll" criterion: the dev pass keeps each minibatch's
probs and targets on the device (R_dev x D x 4 bytes of probabilities, and as much again for fp32 targets), calls
FusedMLP.ranking ONCE over all of them at the end -- rank metrics are not additive over minibatches -- and logs `dev_auroc` and
`dev_avg_precision`, the macro means of the per-label AUROC and average precision ("nll": each class against the rest).

opt.conformal_levels = [level, ...] (off by default) with opt.predictive and the NLL criterion: the dev pass keeps each
minibatch's probs and targets on the device, calibrates split conformal prediction on the FIRST half of the dev rows
(FusedMLP.conformal_calibrate, opt.conformal_score = "aps" by default, or "lac") and logs, from the sets of the SECOND half
(FusedMLP.conformal_sets), `dev_cov@<level>` (the fraction of sets that hold the target; at least the level in expectation)
and `dev_set_size@<level>` (the mean number of classes in a set).

opt.conformal_interval_levels = [level, ...] (off by default) with opt.predictive and a regression criterion ("mse" / "gauss"):
the dev pass keeps each minibatch's result and targets on the device, calibrates split conformal intervals on the FIRST half of the
dev rows (FusedMLP.conformal_calibrate_intervals; opt.conformal_interval_score = "scaled" by default, "absolute", or "cqr", which
needs opt.quantile_probs to hold both probabilities of every level; opt.conformal_interval_scope = "per_output" by default, or
"joint") and logs, from the intervals of the SECOND half (FusedMLP.conformal_intervals), `dev_icov@<level>` (the fraction of the
targets inside their interval; at least the level in expectation) and `dev_iwidth@<level>` (the mean width hi - lo).

opt.criterion = "bce" (the Bernoulli likelihood: multi-label classification, binary with one label): targets are R x D fp32
labels, the accuracy is the label accuracy 100 correct / (rows S D), and with opt.predictive the dev pass calls
FusedMLP.predict_labels and logs `devll_pred` (the joint log-likelihood of a row's label vector), `dev_label_acc`,
`dev_exact_match` and `dev_label_mi` (the mean per-label mutual information).

Differences from main.lua, all deliberate: the loop ends after `epochs` (the reference loops forever, :164); a last
short minibatch is skipped rather than padded with uninitialised rows (data.lua:9-20); targets are 0-based.
"""
import os

import numpy as np
import torch

from . import checkpoint as ckpt
from . import utils as u
from .engine import FusedMLP
from .logger import Logger

# the series VBLinear:update logs per layer and minibatch, in the order of its Log:add calls (VBLinear.lua:149-164)
UPDATE_SERIES = ("vlc grad", "vle grad", "mlc grad", "mle grad", "min variance", "max variance", "mean variance", "var hat",
                 "mean means", "std means", "min. means", "max. means", "mu normratio", "var normratio")


def default_opt(**over):
    """config.lua's values under the engine's key names (config.lua:5-68)."""
    opt = {
        "network_name": "exp", "type": "vb", "dataset": "mnist",
        "batchSize": 100, "testBatchSize": 100, "trainSize": 100, "testSize": 1000,     # config.lua:11-16 (batchSize 1 there)
        "geometry": (28, 28), "input_size": 784, "n_classes": 10, "hidden": [10],        # :17-18, :31
        "B": 1e6, "S": 30, "testSamples": 30, "log": True,                                # :30-35
        "seed": 3, "mu_init": 0, "var_init": 1e-3,                                        # :40-44
        "state": {"learningRate": 1e-3}, "varState": {"learningRate": 5e-2}, "meanState": {"learningRate": 1e-4},  # :51-64
        "mode": "lrt", "dtype": "f32", "fuse_kl": True,
    }
    opt.update(over)
    return opt


class Main:
    def __init__(self, opt, device=None, net=None):
        # (the KL gradient: FusedMLP's own default -- exact, from the fp32 parameters in the update sweep wherever the fused
        # epilogue would read bf16 shadows; the saved opt records the form that actually ran)
        self.net = net or FusedMLP(opt, device=device)
        self.opt = dict(opt, kl_in_update=bool(getattr(self.net, "kl_in_update", False)))
        self.device = self.net.device
        self.rng = np.random.RandomState(int(opt.get("seed", 3)))                         # torch.manualSeed(3), config.lua:40
        self.indices = None
        self.epoch = 0                                                                    # epochs run so far (opt.prune_schedule counts them)
        self.log = Logger(opt["network_name"], append=bool(opt.get("network_to_load"))) if opt.get("log") else None
        if opt.get("network_to_load"):                                                    # main.lua:146-148
            self._resume(os.path.join(str(opt["network_to_load"]), "model"))

    def _resume(self, path):
        """opt.network_to_load = <dir>: <dir>/model (a FusedMLP.save file, written by a run with opt.checkpoint) goes into this Main's engine;
        its `trainer` table, when it has one, restores the epoch counter (opt.prune_schedule continues at the right epoch), the minibatch
        start indices and the shuffling RandomState. A file without one resumes the engine only."""
        if not os.path.isfile(path):
            raise FileNotFoundError(f"opt.network_to_load: {path} does not exist (a run saves it with opt.checkpoint = True)")
        table = ckpt.read_checkpoint(path)
        self.net.load_state_dict(table["engine"])
        tr = table.get("trainer")
        if tr:
            self.epoch = int(tr["epoch"])
            idx = np.asarray(tr["indices"]).astype(np.int64).reshape(-1).tolist()
            self.indices = idx if idx else None
            ckpt.rng_from_table(tr["rng"], self.rng)

    def _to_device(self, inputs, targets):
        x = torch.from_numpy(np.ascontiguousarray(inputs, dtype=np.float32)).to(self.device)
        regression = getattr(self.net, "criterion", "nll") in ("mse", "gauss", "bce")    # R x D fp32 targets; class labels otherwise
        t = torch.from_numpy(np.ascontiguousarray(targets)).to(self.device, dtype=torch.float32 if regression else torch.int32)
        return x, t

    def train(self, dataset):                                                             # main.lua:12-50
        opt, net = self.opt, self.net
        bs, n = int(opt["batchSize"]), int(opt["trainSize"])
        S = int(opt["S"]) if opt.get("type", "vb") == "vb" else 1
        if self.indices is None:
            self.indices = list(range(0, n - bs + 1, bs))                                 # torch.range(1, trainSize, batchSize)
        accuracy = error = 0.0
        net.prepare()                     # once: afterwards update() maintains the operand shadows and prior statistics
        stacked = net.mode == "lrt" and S > 1 and bool(opt.get("stack_draws", True))
        for batch_index in u.shuffle(self.indices, self.rng):
            inputs, targets = dataset.create_minibatch(batch_index, bs, n, opt.get("geometry"))
            x, t = self._to_device(inputs, targets)
            net.resetGradients()
            if stacked:                                                                   # main.lua:32-37 as rows of one pass
                net.run_draws(x, t, S)
            else:
                for _ in range(S):
                    net.sample()
                    net.run(x, t)
            loss, correct = net.loss_and_accuracy()           # sums over the S draws (the criterion accumulates)
            if not np.isfinite(loss):
                # Divergence must be seen HERE: the bf16 gradInput epilogue carries the ReLU mask through its second pass as a
                # NaN and zeroes every NaN it reads back (csrc/epilogues.h, EpiDx::apply_folded), so a genuine NaN above a layer
                # does not reach the layers below it the way model:backward propagates it in the reference (mlp.lua:79) -- the
                # loss and the last layer's gradients still show it (tests: test_nan_in_the_backward_...). No update on such a step.
                raise FloatingPointError(f"minibatch {batch_index}: the loss is {loss} -- the run has diverged; no parameter was updated")
            error += loss * net.world / S
            labels = net.n_classes if getattr(net, "criterion", "nll") == "bce" else 1    # "bce" counts label hits: rows x S x D
            accuracy += 100.0 * correct / (bs * S * labels)
            log_update = bool(self.log and opt.get("log_update") and net.mode == "lrt")
            net.update(opt, log=log_update)
            if log_update:                                                                # VBLinear.lua:149-164, per layer
                for row in net.update_log.cpu().tolist():
                    for name, value in zip(UPDATE_SERIES, row):
                        self.log.add(name, value)
        B = len(self.indices)
        return accuracy / B, error / B

    def test(self, dataset):                                                              # main.lua:52-69
        opt, net = self.opt, self.net
        bs, n = int(opt["testBatchSize"]), int(opt["testSize"])
        starts = list(range(0, n - bs + 1, bs))
        accuracy = error = 0.0
        criterion = getattr(net, "criterion", "nll")
        regression = criterion in ("mse", "gauss")
        # opt.predictive with a regression criterion: the predictive log-likelihood (gauss: the network's own noise; mse: only
        # with opt.noise_var), the epistemic variance and, for gauss, the aleatoric one -- FusedMLP.predict_regression
        tau2 = opt.get("noise_var") if criterion == "mse" else None
        pred = {"devacc_pred": 0.0, "devnll_pred": 0.0, "dev_mi": 0.0}
        if criterion == "bce":            # the multi-label predictive (FusedMLP.predict_labels)
            pred = {"devll_pred": 0.0, "dev_label_acc": 0.0, "dev_exact_match": 0.0, "dev_label_mi": 0.0}
        if regression:
            pred = {"dev_epi_var": 0.0}
            if criterion == "gauss":
                pred.update(devll_pred=0.0, dev_noise_var=0.0)
            elif tau2 is not None:
                pred["devll_pred"] = 0.0
        # opt.quantile_probs (off by default): `dev_cal@<p>`, the fraction of the test targets at or below the predictive's
        # p-quantile (calibrated: p) -- FusedMLP.predict_quantiles, whose moments are predict_regression's of the same draws
        qprobs = [float(v) for v in (opt.get("quantile_probs") or [])] if (regression and opt.get("predictive")) else []
        # opt.predictive = "analytic": the same series from FusedMLP.predict_analytic -- one moment-propagation pass instead of
        # opt.testSamples forwards ("mse" and "nll"; it has no quantiles)
        analytic = opt.get("predictive") == "analytic"
        if analytic and qprobs:
            raise ValueError("opt.quantile_probs needs the sampled predictive (opt.predictive = True): predict_analytic has no quantiles")
        for pj in qprobs:
            pred[f"dev_cal@{pj:g}"] = 0.0
        # opt.calibration_bins = M (0 = off, the default) with a class predictive: ONE CalibrationResult accumulated over the dev
        # minibatches on the device (FusedMLP.calibration, into=) gives `dev_ece`, `dev_mce`, `dev_brier`; opt.selective_coverages
        # adds `dev_acc@cov<c>`, the accuracy over the fraction c of the rows the predictive entropy ranks most certain
        # (FusedMLP.selective). Both need the R x C probabilities, which the predictive then keeps.
        cal_bins = int(opt.get("calibration_bins") or 0) if (opt.get("predictive") and not regression and criterion != "bce") else 0
        cal = None
        # opt.ranking (off by default) with a "bce" or "nll" predictive: every minibatch's probs and targets are kept on the device
        # (R_dev x D x 4 bytes of probabilities) and ranked ONCE after the pass (FusedMLP.ranking): `dev_auroc`, `dev_avg_precision`
        ranking = bool(opt.get("ranking")) and bool(opt.get("predictive")) and not regression
        rank_probs, rank_targets = [], []
        # opt.conformal_levels (off by default) with a class predictive: calibrated on the first half of the dev rows, measured
        # on the second (FusedMLP.conformal_calibrate / conformal_sets): `dev_cov@<level>`, `dev_set_size@<level>`
        conf_levels = [float(v) for v in (opt.get("conformal_levels") or [])] if (opt.get("predictive") and not regression and criterion != "bce") else []
        conf_probs, conf_targets = [], []
        # opt.conformal_interval_levels (off by default) with a regression predictive: calibrated on the first half of the dev rows,
        # measured on the second (FusedMLP.conformal_calibrate_intervals / conformal_intervals): `dev_icov@<level>`,
        # `dev_iwidth@<level>`
        ci_levels = [float(v) for v in (opt.get("conformal_interval_levels") or [])] if (opt.get("predictive") and regression) else []
        ci_score = opt.get("conformal_interval_score") or "scaled"
        ci_results, ci_targets = [], []
        if ci_levels:                                        # refused here, not after a pass of predictions
            from .conformal import check_interval_options
            if ci_score == "cqr" and analytic:
                raise ValueError("opt.conformal_interval_score = 'cqr' needs the sampled predictive (opt.predictive = True): "
                                 "predict_analytic has no quantiles")
            check_interval_options("opt.conformal_interval_levels", ci_levels, ci_score, opt.get("conformal_interval_scope") or "per_output",
                                   torch.tensor(qprobs, dtype=torch.float32).tolist() if ci_score == "cqr" else None)
        for t0 in starts:
            inputs, targets = dataset.create_minibatch(t0, bs, n, opt.get("geometry"))
            x, t = self._to_device(inputs, targets)
            err, acc = net.test(x, t)
            accuracy += acc
            error += err
            if opt.get("predictive") and criterion == "bce":
                if analytic:
                    raise ValueError("opt.predictive = 'analytic' does not support criterion = 'bce' yet: use opt.predictive = True "
                                     "(predict_labels)")
                r = net.predict_labels(x, targets=t)
                pred["devll_pred"] += r.log_lik
                pred["dev_label_acc"] += r.label_accuracy
                pred["dev_exact_match"] += r.exact_match
                pred["dev_label_mi"] += float(r.mutual_info.double().mean())
                if ranking:
                    rank_probs.append(r.probs)
                    rank_targets.append(t)
            elif opt.get("predictive") and regression:
                if analytic:
                    r = net.predict_analytic(x, targets=t, noise_var=tau2)
                elif qprobs:                                 # opt.quantile_probs: the same draws give the calibration too
                    qr = net.predict_quantiles(x, qprobs, targets=t, noise_var=tau2)
                    r = qr.moments
                    for pj, cj in zip(qprobs, qr.calibration):
                        pred[f"dev_cal@{pj:g}"] += cj
                else:
                    r = net.predict_regression(x, targets=t, noise_var=tau2)
                pred["dev_epi_var"] += r.mean_var
                if "devll_pred" in pred:
                    pred["devll_pred"] += r.log_lik
                if "dev_noise_var" in pred:
                    pred["dev_noise_var"] += r.mean_noise_var
                if ci_levels:
                    ci_results.append(qr if (qprobs and not analytic) else r)
                    ci_targets.append(t)
            elif opt.get("predictive"):    # the S-draw model average on the same minibatch (its own draws, after test()'s)
                if analytic:
                    r = net.predict_analytic(x, targets=t, keep_probs=bool(cal_bins) or ranking or bool(conf_levels))
                elif getattr(net, "n_classes", 0) > 16:      # predict's head holds a row's classes in one 16-wide tile
                    r = net.predict_classes(x, targets=t, keep_probs=bool(cal_bins) or ranking or bool(conf_levels))
                else:
                    r = net.predict(x, targets=t)
                if cal_bins:
                    cal = net.calibration(r, t, bins=cal_bins, into=cal)
                pred["devacc_pred"] += r.accuracy
                pred["devnll_pred"] += r.nll
                pred["dev_mi"] += float(r.mutual_info.double().mean())
                if ranking:
                    rank_probs.append(r.probs)
                    rank_targets.append(t)
                if conf_levels:
                    conf_probs.append(r.probs)
                    conf_targets.append(t)
        self.predictive = {k: v / len(starts) for k, v in pred.items()} if opt.get("predictive") else None
        if cal is not None:                                  # (sums over the whole dev set, not means of minibatch values)
            self.predictive.update(dev_ece=cal.ece, dev_mce=cal.mce, dev_brier=cal.brier)
            covs = [float(c) for c in (opt.get("selective_coverages") or [])]
            if covs:
                sel = net.selective(cal.entropy, cal.hit, covs)
                self.predictive.update({f"dev_acc@cov{c:g}": a for c, a in zip(covs, sel.accuracy)})
        if ranking and rank_probs:                           # (one call over the whole dev set: ranks do not add)
            rk = net.ranking(rank_probs, rank_targets)
            self.predictive.update(dev_auroc=rk.macro_auroc, dev_avg_precision=rk.macro_average_precision)
        if conf_levels and conf_probs:
            P, T = torch.cat(conf_probs), torch.cat(conf_targets)
            h = P.shape[0] // 2
            if h >= 1:
                cc = net.conformal_calibrate(P[:h], T[:h], levels=conf_levels, score=opt.get("conformal_score") or "aps")
                cs = net.conformal_sets(P[h:], cc, targets=T[h:])
                for lv, cov, sz in zip(conf_levels, cs.coverage, cs.mean_size):
                    self.predictive[f"dev_cov@{lv:g}"] = cov
                    self.predictive[f"dev_set_size@{lv:g}"] = sz
        if ci_levels and ci_results:
            from .conformal import split_rows
            h = sum(t.shape[0] for t in ci_targets) // 2
            if h >= 1:
                (r1, t1), (r2, t2) = split_rows(ci_results, ci_targets, h)
                ic = net.conformal_calibrate_intervals(r1, t1, levels=ci_levels, score=ci_score,
                                                       scope=opt.get("conformal_interval_scope") or "per_output",
                                                       noise_var=(tau2 or None) if (criterion == "mse" and ci_score == "scaled") else None)
                ir = net.conformal_intervals(r2, ic, targets=t2)
                for lv, cov, wd in zip(ci_levels, ir.coverage, ir.mean_width):
                    self.predictive[f"dev_icov@{lv:g}"] = cov
                    self.predictive[f"dev_iwidth@{lv:g}"] = wd
        return accuracy / len(starts), error / len(starts)

    def _prune_series(self, testSet):
        """opt.prune_report = T: the two numbers mainviz.lua:22-27 prints at threshold T (`pruned count`, `pruned var mean`), from
        the device (FusedMLP.prune). opt.prune_eval = [fractions]: `devacc_pruned@<q>`, the accuracy of the MAP prediction over
        the test set with the fraction q of the weights pruned globally (FusedMLP.prune_curve per test minibatch)."""
        opt, net, rec = self.opt, self.net, {}
        if opt.get("prune_report") is not None:
            r = net.prune(threshold=float(opt["prune_report"]))
            rec["pruned count"], rec["pruned var mean"] = r.n_pruned, r.mean_pruned_var
        qs = list(opt.get("prune_eval") or [])
        if qs:
            bs, n = int(opt["testBatchSize"]), int(opt["testSize"])
            starts = list(range(0, n - bs + 1, bs))
            acc = [0.0] * len(qs)
            for t0 in starts:
                inputs, targets = testSet.create_minibatch(t0, bs, n, opt.get("geometry"))
                x, t = self._to_device(inputs, targets)
                for j, row in enumerate(net.prune_curve(x, t, qs, map=True)):
                    acc[j] += row["accuracy"]
            for q, a in zip(qs, acc):
                rec[f"devacc_pruned@{q:g}"] = a / len(starts)
        return rec

    def start_epoch(self):
        """What run() does before an epoch's training: opt.prune_schedule's entries for the epoch about to start --
        prune(fraction, opt.prune_scope), then hold_pruned -- and the epoch counter. Public so that a caller that drives train()
        itself (tools/finetune_bench.py measures between the pruning and the training) follows the same schedule."""
        for epoch, fraction in (self.opt.get("prune_schedule") or []):
            if int(epoch) == self.epoch:
                res = self.net.prune(fraction=float(fraction), scope=self.opt.get("prune_scope", "global"))
                self.net.hold_pruned(res)
        self.epoch += 1

    def save(self):
        """The run directory's data files (mainviz.lua:11-15): every VB layer's means / vars flattened and
        concatenated in layer order -- the order of the reference's flat `parameters` vector (mlp.lua:37)."""
        net, d = self.net, self.opt["network_name"]
        means = torch.cat([v.means.reshape(-1) for v in net.vb]).cpu().numpy()
        vars_ = torch.cat([v.lvars.reshape(-1) for v in net.vb]).exp().cpu().numpy()
        u.safe_save(means, os.path.join(d, "parameters"), "means")
        u.safe_save(vars_, os.path.join(d, "parameters"), "vars")
        u.safe_save({k: (list(v) if isinstance(v, tuple) else v) for k, v in self.opt.items()}, d, "opt")
        if self.opt.get("checkpoint"):
            # main.lua:181's `model`, as data: the engine's whole state and the trainer's, one file (checkpoint.py). The replicas of a
            # data-parallel run are compared first (a collective: every rank is here); rank 0 alone writes
            net.check_replicas()
            if getattr(net, "rank", 0) == 0:
                net.save(os.path.join(d, "model"), trainer={"epoch": self.epoch, "indices": self.indices,
                                                            "rng": ckpt.rng_state_table(self.rng)})

    def run(self, trainSet, testSet, epochs=1):                                           # main.lua:138-184
        history = []
        for _ in range(epochs):
            self.start_epoch()                                                             # opt.prune_schedule (off by default)
            trainAccuracy, trainError = self.train(trainSet)
            testAccuracy, testError = self.test(testSet)
            rec = {"devacc": testAccuracy, "trainacc": trainAccuracy, "deverr": testError, "trainerr": trainError}
            if getattr(self, "predictive", None):                                          # opt.predictive
                rec.update(self.predictive)
            if getattr(self.net, "sharded", False):
                self.net.gather_parameters()              # collective (every rank runs this loop): calc_lc and save read fp32 rows
            if self.opt.get("type", "vb") == "vb":
                rec["lc"] = self.net.calc_lc(self.opt)
            if self.opt.get("prune_schedule"):
                held = self.net.held
                rec["held fraction"] = (sum(held) / sum(v.O * v.I for v in self.net.vb)) if held else 0.0
            rec.update(self._prune_series(testSet))       # opt.prune_report / opt.prune_eval (both off by default)
            if self.log:
                for k in ("devacc", "trainacc", "deverr", "trainerr", "lc", "devacc_pred", "devnll_pred", "dev_mi", "devll_pred", "dev_epi_var",
                          "dev_noise_var", "dev_ece", "dev_mce", "dev_brier", "dev_auroc", "dev_avg_precision"):   # main.lua:169-177 (+ opt.predictive, opt.calibration_bins, opt.ranking)
                    if k in rec:
                        self.log.add(k, rec[k])
                for k in rec:
                    if k in ("pruned count", "pruned var mean", "held fraction") or k.startswith(("devacc_pruned@", "dev_cal@", "dev_acc@cov", "dev_cov@", "dev_set_size@", "dev_icov@", "dev_iwidth@")):
                        self.log.add(k, rec[k])
                self.log.flush()
                self.save()                                                                # main.lua:181
            history.append(rec)
        return history
