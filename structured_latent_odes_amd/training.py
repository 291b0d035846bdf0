"""Shared body of the three entry points (training_cvs.py / training_proc.py / training_challenge.py of the reference):
``train(config)`` with the reference's structure -- two SVI objects sharing one Adam (training_cvs.py:226-249), an epoch loop of
``run_batch`` (:147-157, :256-266), the four statistics passes per epoch (validation / training x posterior / prior: ``evaluate_loss`` +
``recon`` + label prediction, :43-144, :270-315), best-model copy (:325-331), the per-epoch summary line (:336-352) and the final
test passes on the best model (:355-397).  Batches come from ``synthetic.synthetic_batch`` unless ``--data-dir`` points at
the reference's data files (cvs: ``processed_data.pkl`` ...; challenge: ``data.pkl``; proc: the plate-reader CSVs), which are then read by ``data.py`` (SURVEY row
N3) and fed through pinned host buffers, or the caller passes its own list of batch dicts."""
from __future__ import annotations

import logging
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .svi import SVI, Adam, Trace_ELBO
from .synthetic import synthetic_batch
from .utils.utils import set_seed

FAMILY_LABELS = {"cvs": ("iext", "rtpr"), "challenge": ("symptoms", "shedding"), "proc": ("aR", "aS", "C12", "C6")}


def batch_to_device(d: Dict[str, torch.Tensor], device, family: str) -> Dict[str, torch.Tensor]:
    """training_cvs.py:18-27 / training_proc.py:25-33 / training_challenge.py:27-33: labels -> [B, dim]; cvs/challenge
    observations [B,T,C] -> the [B,C,T] permuted view (no copy); proc observations are already [B,C,T]."""
    out = {}
    for l in FAMILY_LABELS[family]:
        v = d[l]
        out[l] = (v.reshape(v.shape[0], -1) if v.dim() > 1 else v.reshape(-1, 1)).to(device)
    obs = d["observations"]
    out["observations"] = obs.to(device)
    return out


def run_batch(batch, losses) -> List[float]:
    """training_cvs.py:147-157."""
    B = batch["observations"].shape[0]
    return [loss.step(**batch) / B for loss in losses]


def input_pred_stats(batches, model, losses, is_post: bool, device, family: str):
    """training_cvs.py:43-144 without the plotting: -ELBO per trajectory for every loss, reconstruction L1, label predictions."""
    total_elbo, total_l1, size = [0.0] * len(losses), 0.0, 0
    hits = {l: 0.0 for l in FAMILY_LABELS[family]}
    predict = getattr(model, "classifier", None) or model.pred_inputs
    for batch in batches:
        batch = batch_to_device(batch, device, family)
        B = batch["observations"].shape[0]
        for i, loss in enumerate(losses):
            total_elbo[i] += loss.evaluate_loss(**batch) / B
        total_l1 += float(model.recon(is_post=is_post, **batch)["l1"])
        pred = predict(observations=batch["observations"])
        for l in hits:
            if pred[l].shape == batch[l].shape:
                hits[l] += float((pred[l] - batch[l]).abs().lt(0.5).all(dim=1).float().sum())
        size += B
    out = {l: hits[l] / max(size, 1) for l in hits}
    out.update(l1=total_l1 / max(size, 1), elbo=torch.tensor(total_elbo))
    return out


STATS_CHUNK = 64   # rows by which the table of a fused statistics pass grows when the batch source has no len()


def _to_host(table: torch.Tensor) -> np.ndarray:
    """THE device-to-host copy of a fused statistics pass (float64 on the host)."""
    return table.detach().cpu().double().numpy()


def input_pred_stats_fused(batches, model, is_post: bool, device, family: str, num_particles: int = 1):
    """``input_pred_stats`` with one engine call per batch and ONE read-back per pass: every batch writes its row of sums
    (``model.eval_stats``: -ELBO main, auxiliary loss, reconstruction L1 sum, hits per label, B) into a device table; the table comes back
    once, at the end, and the pass is summed on the host in float64.  Same dict, same arithmetic quirks of the reference: ``elbo`` is the sum
    over batches of loss / B, ``l1`` the sum of the per-batch means over the number of trajectories."""
    from . import _lib as L
    n = len(batches) if hasattr(batches, "__len__") else STATS_CHUNK
    table = torch.empty(max(n, 1), L.EVAL_SLOTS, dtype=torch.float32, device=device)
    elems, i = [], 0
    for batch in batches:
        batch = batch_to_device(batch, device, family)
        if i == table.shape[0]:
            grown = torch.empty(i + STATS_CHUNK, L.EVAL_SLOTS, dtype=torch.float32, device=device)
            grown[:i].copy_(table)
            table = grown
        obs = batch["observations"]
        model.eval_stats(is_post=is_post, out=table[i], num_particles=num_particles, **batch)
        elems.append(obs.shape[1] * obs.shape[2])
        i += 1
    rows = _to_host(table[:i]) if i else np.zeros((0, L.EVAL_SLOTS))
    B = rows[:, L.EVAL_SLOTS - 1]
    size = float(B.sum())
    slots = model.eval_stat_slots()
    out = {l: (float(rows[:, slots[l]].sum()) if l in slots else 0.0) / max(size, 1) for l in FAMILY_LABELS[family]}
    l1 = float((rows[:, 2] / (B * np.asarray(elems, dtype=np.float64))).sum()) if i else 0.0
    out.update(l1=l1 / max(size, 1), elbo=torch.tensor([float((rows[:, 0] / B).sum()), float((rows[:, 1] / B).sum())]))
    return out


def make_batches(config, family: str, n_batches: int, seed: int):
    out = []
    for i in range(n_batches):
        obs, labels, _ = synthetic_batch(family, config.mini_batch_size, config.seq_len, config.obs_dim, seed=seed + i)
        d = {"observations": obs}
        d.update(labels)
        out.append(d)
    return out


def train(config, family: str, model_cls, model_cls_gauss, batches_per_epoch: int = 7,
          train_batches: Optional[Sequence[dict]] = None, val_batches: Optional[Sequence[dict]] = None, times: Optional[torch.Tensor] = None,
          test_batches: Optional[Sequence[dict]] = None, fused_stats: bool = False, sample_moments: bool = False,
          results_dir: Optional[str] = None, test_bounds: int = 0, forecast_steps: int = 0, cohort_curves: bool = False, calibration: bool = False,
          label_evidence: int = 0, refine_steps: int = 0, refine_draws: int = 8, waic: int = 0, attribution: int = 0,
          curve_summary: int = 0, summary_thresholds=None, summary_sense: str = "above", sample_quantiles: int = 0,
          quantile_levels=(0.025, 0.975), mechanism: int = 0, joint_band: int = 0, band_levels=(0.95,), loo: int = 0,
          intervention_summary: int = 0, forecast_summary: int = 0):
    """fused_stats: the four statistics passes of every epoch run through ``input_pred_stats_fused`` (one engine call per batch, one
    read-back per pass) instead of ``input_pred_stats``.  The final test passes score two models at once (the losses stay bound to
    var_model while recon / label prediction run on best_model, as in the reference) and keep the unfused form.
    sample_moments: after the final test passes, the reference's ``multiple_samples`` stage (training_proc.py:205-223) on the first test
    batch, posterior and prior, config.num_samples draws -- as ``save_recon_moments`` (mean and sd over the draws per curve, written to
    ``results_dir``, default ``results_<config.model>``); off by default: no such stage runs.
    test_bounds = K > 0: after training, the best model's per-trajectory bounds from K posterior draws (``save_trajectory_bounds``: -ELBO,
    importance-weighted bound, effective sample size, mean NLL) over the validation loader, written to ``results_dir`` as
    ``bounds_post.npy`` [n, 4]; 0 (the default): no such stage runs.
    forecast_steps = N > 0: after training, the best model's posterior forecast over the validation loader on ``horizon_times(N)`` -- the
    training grid and N more steps of its last spacing -- mean and sd over config.num_samples draws per curve, the trajectories in loader
    order, written to ``results_dir`` under ``save_forecast_moments``' file names; 0 (the default): no such stage runs.
    cohort_curves: after training, the per-condition curves of the reference's evaluation notebooks on the first test batch -- cohorts
    from all of the family's labels, posterior and prior, config.num_samples draws (``save_cohort_moments``) -- and the notebooks' number,
    printed as ``l1_error_post`` / ``l1_error_prior``: the mean of ``l1`` over non-empty cohorts and channels; off by default.
    calibration: after training, the best model's calibration pass over the validation loader, posterior and prior, config.num_samples
    draws, the whole loader as one cohort (``save_calibration``: coverage of every curve against its nominal level, band coverage, crossing
    share, pinball loss), one printed line per side (``calibration_post: ...``); off by default.
    label_evidence = K > 0: after training, the best model's own label posterior p(u | x) ~ p(u) p(x | u) over the validation loader from K
    posterior draws (``save_label_evidence`` on ``default_hypotheses``: ``evidence_post.npy`` [n, V, 4], ``evidence_best.npy``,
    ``evidence_match.npy``, ``evidence_hypotheses_<label>.npy``) and one printed line (``label_evidence: ...``: the share of subjects whose
    most probable hypothesis is their own labels, the mean posterior mass there, the median ESS there) beside the classifier accuracies;
    0 (the default): no such stage runs.
    refine_steps = J > 0: after training, the best model's posterior refined subject by subject over the validation loader -- J Adam steps
    per trajectory on its own (loc, log scale) against its ``refine_draws``-draw -ELBO (``save_refined_posterior``: ``refined_loc.npy``,
    ``refined_scale.npy``, ``refined_elbo.npy`` [n, 2]) -- and one printed line (``refine_posterior: ...``: the mean -ELBO before and after);
    0 (the default): no such stage runs.
    waic = K > 0: after training, the best model's pointwise predictive density over the validation loader from K posterior draws
    (``save_pointwise_density``: ``pointwise_{lppd,p_waic,mean_ll}_post.npy`` [n, C, T], ``waic_post.npy`` [n, 8]) and one printed line
    (``waic: ...``: total elpd_waic and its standard error over trajectories, total p_waic, the share of points with p_waic > 0.4);
    loo = K > 0: after training, the best model's PSIS leave-one-out over the validation loader from K posterior draws
    (``save_pointwise_loo``: ``pointwise_{elpd_loo,khat}_post.npy`` [n, C, T], ``loo_post.npy`` [n, 8]) and one printed line (``loo: ...``:
    total elpd_loo and its standard error over trajectories, total p_loo, the shares of points with khat > 0.7 and > 0.5);
    0 (the default): no such stage runs.
    attribution = K > 0: after training, the best model's latent attribution over the validation loader from K pick-freeze draws, posterior
    and prior (``save_latent_attribution``: ``attribution_{total,first}[_index]_<post|prior>.npy``, ``attribution_blocks.txt``) and one
    printed line per side (``attribution_post: ...``: per latent block, the mean total and first-order index); 0 (the default): no such
    stage runs.
    curve_summary = K > 0: after training, the best model's curve summaries over the validation loader from K draws, posterior and prior
    (``save_curve_summary``: ``summary_<curve>_<post|prior>_{mean,sd}.npy`` [n, C, 8], ``summary_slots.npy``) and one printed line per side
    (``curve_summary_post: ...``: per channel of the central curve, the mean peak, time to peak and AUC and, with ``summary_thresholds`` --
    one level per channel, ``summary_sense`` "above" or "below" --, P(cross) and the mean t_hit); 0 (the default): no such stage runs.
    sample_quantiles = K > 0: after training, the best model's sample quantiles at ``quantile_levels`` over the validation loader from K
    draws, posterior and prior (``save_recon_quantiles``: ``<curve>_<post|prior>_sample_quantiles.npy`` [n, Lv, C, T],
    ``sample_quantile_levels.npy``) and one printed line per side (``sample_quantiles_post: ...``: the mean width of the band between the
    lowest and the highest level of the central curve and the share of observation points inside it); 0 (the default): no such stage runs.
    mechanism = K > 0: after training, the best model's mechanism curves over the validation loader from K draws, posterior and prior
    (``save_mechanism_moments``: ``mechanism_<name>_<post|prior>_{mean,sd}.npy`` [n, T, S] for the state, production, degradation, set point
    and net rate) and one printed line per side (``mechanism_post: ...``: per state component, the time-averaged mean production,
    degradation and set point); 0 (the default): no such stage runs.
    joint_band = K > 0: after training, the best model's simultaneous (sup-t) bands at ``band_levels`` over the validation loader from K
    draws, posterior and prior (``save_simultaneous_band``: ``<curve>_<post|prior>_band_{mean,sd,crit,pointwise_joint,obs_dev}.npy``,
    ``band_levels.npy``) and one printed line per side (``joint_band_post: ...``: per level of the central curve, the mean critical value
    beside the pointwise z, the mean share of draws wholly inside the pointwise band and the share of subject-channels whose observation
    lies wholly inside the simultaneous band); 0 (the default): no such stage runs.
    intervention_summary = K > 0: after training, the best model's counterfactual summaries over the validation loader from K paired
    posterior draws on ``default_hypotheses`` (``save_intervention_summary``: ``summary_<curve>_{factual,cf,effect}_{mean,sd}.npy``,
    ``summary_hypotheses_<label>.npy``), with ``summary_thresholds`` / ``summary_sense`` as for ``curve_summary``, and one printed line per
    hypothesis (``intervention_summary: ...``: per channel of the central curve, the mean paired effect on the peak and on the AUC and, with
    thresholds, the change of P(cross)); 0 (the default): no such stage runs.
    forecast_summary = K > 0 (needs ``forecast_steps`` = N > 0): after training, the best model's forecast summaries over the validation
    loader from K posterior draws on ``horizon_times(N)``, taken from the model's last training time on (``save_forecast_summary``:
    ``summary_<curve>_post_forecast_{mean,sd}.npy`` [n, C, 8], ``forecast_times.npy``), with ``summary_thresholds`` / ``summary_sense`` as
    for ``curve_summary``, and one printed line per head curve (``forecast_summary_<curve>: ...``: per channel, the mean future peak and,
    with thresholds, P(cross) and the mean t_hit over the subjects with a crossing draw); 0 (the default): no such stage runs."""
    if forecast_summary and not forecast_steps:
        raise ValueError("forecast_summary needs forecast_steps > 0 (the horizon to summarise)")
    set_seed(config.seed)
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if times is not None:
        times = times.to(device)
    elif family == "proc":
        _, _, times = synthetic_batch("proc", 1, config.seq_len, config.obs_dim, seed=0)     # non-uniform grid like the CSV times
        times = times.to(device)
    else:
        times = torch.arange(0.0, end=config.seq_len * config.delta_t, step=config.delta_t, device=device)
    if config.model == "Mechanistic":
        selected = model_cls
    elif config.model == "MechanisticGauss":
        selected = model_cls_gauss
    else:
        raise ValueError("selected model is not implemented")
    var_model = selected(config=config, device=device, times=times).to(device)
    msg = "Model: %s -  with %d parameters." % (config.model, sum(p.numel() for p in var_model.parameters()))
    print(msg)
    logging.debug(msg)
    best_model = selected(config=config, device=device, times=times).to(device)
    optimizer = Adam({"lr": config.learning_rate, "betas": (0.9, 0.999)})
    elbo = Trace_ELBO(num_particles=config.num_particles)
    losses = [SVI(var_model.model, var_model.guide, optimizer, loss=elbo),
              SVI(var_model.model_meta, var_model.guide_meta, optimizer, loss=elbo)]
    # batch sources may be lists or re-iterable feeders (data.BatchFeeder: a fresh pass, reshuffled, every epoch)
    train_b = train_batches if train_batches is not None else make_batches(config, family, batches_per_epoch, seed=1000)
    val_b = val_batches if val_batches is not None else make_batches(config, family, 1, seed=5000)
    test_b = test_batches if test_batches is not None else val_b          # cvs ships a test split; challenge / proc test on the validation fold
    best_val_loss, best_epoch = np.inf, 0
    names = FAMILY_LABELS[family][:2]
    for epoch in range(config.num_epochs + 1):
        t_ep, n_traj, epoch_loss = time.perf_counter(), 0, []
        for b in train_b:
            d = batch_to_device(b, device, family)
            epoch_loss.append(run_batch(d, losses))          # (every step ends in the .item() of its loss: the clock sees finished work)
            n_traj += d["observations"].shape[0]
        traj_per_s = n_traj / max(time.perf_counter() - t_ep, 1e-9)
        # the reference's four statistics passes per epoch (training_cvs.py:270-315): validation posterior / prior, training
        # posterior / prior -- every one a full pass over its loader: evaluate_loss of both SVI objects, recon, label prediction
        if fused_stats:
            def stats(b, post): return input_pred_stats_fused(b, var_model, post, device, family, config.num_particles)
        else:
            def stats(b, post): return input_pred_stats(b, var_model, losses, post, device, family)
        val = stats(val_b, True)
        _ = stats(val_b, False)
        trn = stats(train_b, True)
        trn_prior = stats(train_b, False)
        val_elbo = torch.sum(val["elbo"]) * len(val["elbo"])
        improved = ""
        if best_val_loss >= val_elbo:
            best_val_loss, best_epoch, improved = val_elbo, epoch, "*"
            best_model.load_state_dict(var_model.state_dict())
        # the reference's summary line (training_cvs.py:336-352) + the training throughput of the epoch: trajectories through
        # run_batch (main + auxiliary SVI step, two Adam passes) per second of wall time, host-to-device copies included
        line = "[Epoch %d/%d] loss= %.4f  %s_acc=(%.4f,%.4f)  %s_acc=(%.4f,%.4f) l1=(%.6f,%.6f), %s  trajectories/sec=%.0f" % (
            epoch, config.num_epochs, float(np.mean(epoch_loss)), names[0], trn[names[0]], val[names[0]], names[1], trn[names[1]],
            val[names[1]], trn["l1"], val["l1"], improved, traj_per_s)
        print(line)
        logging.debug(line)
    # final test passes on the best model, posterior and prior (training_cvs.py:355-397); the losses stay bound to var_model, as there
    test_post = input_pred_stats(test_b, best_model, losses, True, device, family)
    test_prior = input_pred_stats(test_b, best_model, losses, False, device, family)
    final = "FINAL TEST: %s_acc=(%.4f,%.4f)  %s_acc=(%.4f,%.4f) l1=(%.6f,%.6f)" % (
        names[0], test_post[names[0]], test_prior[names[0]], names[1], test_post[names[1]], test_prior[names[1]], test_post["l1"], test_prior["l1"])
    print(final)
    logging.debug(final)
    tail = "ELBO: best_epoch: {} post: {} prior: {}".format(best_epoch, test_post["elbo"], test_prior["elbo"])
    print(tail)
    logging.debug(tail)
    out_dir = results_dir or "results_%s" % config.model
    if sample_moments or cohort_curves or forecast_steps or calibration:      # (the stages that draw; a config without num_samples serves the others)
        num_samples = int(getattr(config, "num_samples", 200))
    if sample_moments:
        d = batch_to_device(next(iter(test_b)), device, family)
        for is_post in (True, False):
            written = best_model.save_recon_moments(out_dir, is_post=is_post, num_samples=num_samples, **d)
            logging.debug("multiple_samples moments: %s", written)
    if cohort_curves:
        d = batch_to_device(next(iter(test_b)), device, family)
        for is_post in (True, False):
            res = best_model.cohort_moments(is_post=is_post, num_samples=num_samples, cohorts=tuple(best_model.LABELS), **d)
            written = best_model._save_arrays(out_dir, best_model._cohort_named(res, is_post))
            line = "l1_error_%s: %s" % ("post" if is_post else "prior", float(res["l1"][res["count"] > 0].mean()))
            print(line)
            logging.debug("%s (%s)", line, written)
    if calibration:
        for is_post in (True, False):
            written, res = best_model.save_calibration(out_dir, (batch_to_device(b, device, family) for b in val_b), is_post, num_samples)
            line = best_model.calibration_line(res, "post" if is_post else "prior")
            print(line)
            logging.debug("%s (%s)", line, written)
    if test_bounds:
        path = best_model.save_trajectory_bounds(out_dir, (batch_to_device(b, device, family) for b in val_b), int(test_bounds))
        logging.debug("per-trajectory bounds: %s", path)
    if label_evidence:
        first = batch_to_device(next(iter(val_b)), device, family)
        hyp = best_model.default_hypotheses(**{l: first[l] for l in best_model.LABELS})
        written = best_model.save_label_evidence(out_dir, (batch_to_device(b, device, family) for b in val_b), int(label_evidence), hyp)
        line = best_model.label_evidence_line(*(np.load(f) for f in written[:3]))
        print(line)
        logging.debug("%s (%s)", line, written)
    if intervention_summary:
        first = batch_to_device(next(iter(val_b)), device, family)
        hyp = best_model.default_hypotheses(**{l: first[l] for l in best_model.LABELS})
        written = best_model.save_intervention_summary(out_dir, (batch_to_device(b, device, family) for b in val_b), int(intervention_summary), hyp,
                                                       thresholds=summary_thresholds, sense=summary_sense)
        central = best_model.MOMENT_HEADS[bool(best_model.GAUSS)][0]
        for line in best_model.intervention_summary_lines(np.load([f for f in written if f.endswith("summary_%s_effect_mean.npy" % central)][0]),
                                                          hyp, summary_thresholds is not None):
            print(line)
            logging.debug("%s", line)
        logging.debug("intervention summary: %s", written)
    if refine_steps:
        written = best_model.save_refined_posterior(out_dir, (batch_to_device(b, device, family) for b in val_b), int(refine_draws), int(refine_steps))
        table = np.load([f for f in written if f.endswith("refined_elbo.npy")][0])
        line = "refine_posterior: J=%d K=%d  n=%d  mean -ELBO before=%.4f after=%.4f" % (
            int(refine_steps), int(refine_draws), table.shape[0], float(table[:, 0].mean()), float(table[:, 1].mean()))
        print(line)
        logging.debug("%s (%s)", line, written)
    if waic:
        written = best_model.save_pointwise_density(out_dir, (batch_to_device(b, device, family) for b in val_b), int(waic))
        line = best_model.waic_line(np.load([f for f in written if os.path.basename(f).startswith("waic_")][0]),
                                    np.load([f for f in written if "p_waic" in f][0]), int(waic))
        print(line)
        logging.debug("%s (%s)", line, written)
    if loo:
        written = best_model.save_pointwise_loo(out_dir, (batch_to_device(b, device, family) for b in val_b), int(loo))
        line = best_model.loo_line(np.load([f for f in written if os.path.basename(f) == "loo_post.npy"][0]),
                                   np.load([f for f in written if "khat" in f][0]), int(loo))
        print(line)
        logging.debug("%s (%s)", line, written)
    # the whole-curve passes, posterior and prior each: (flag value = draws, save method, its keyword arguments, the printed line from
    # load(file-name ending), the central curve's name and the side's tag)
    curve_passes = (
        (attribution, "save_latent_attribution", {}, lambda m, load, central, tag: m.attribution_line(
            load("attribution_total_index_%s.npy" % tag), load("attribution_first_index_%s.npy" % tag), tag)),
        (curve_summary, "save_curve_summary", dict(thresholds=summary_thresholds, sense=summary_sense), lambda m, load, central, tag: m.summary_line(
            load("summary_%s_%s_mean.npy" % (central, tag)), tag, summary_thresholds is not None)),
        (sample_quantiles, "save_recon_quantiles", dict(levels=quantile_levels), lambda m, load, central, tag: m.quantile_line(
            load("%s_%s_sample_quantiles.npy" % (central, tag)), load("sample_quantile_levels.npy"),
            np.concatenate([np.asarray(batch_to_device(b, "cpu", family)["observations"]) for b in val_b], 0), tag)),
        (mechanism, "save_mechanism_moments", {}, lambda m, load, central, tag: m.mechanism_line(
            {k: load("mechanism_%s_%s_mean.npy" % (k, tag)) for k in ("production", "degradation", "set_point")}, tag)),
        (joint_band, "save_simultaneous_band", dict(levels=band_levels), lambda m, load, central, tag: m.band_line(
            *(load("%s_%s_band_%s.npy" % (central, tag, k)) for k in ("crit", "pointwise_joint", "obs_dev")), load("band_levels.npy"), tag)),
    )
    for flag, save, kwargs, line_of in curve_passes:
        for is_post in (True, False) if flag else ():
            written = getattr(best_model, save)(out_dir, (batch_to_device(b, device, family) for b in val_b), is_post, int(flag), **kwargs)
            line = line_of(best_model, lambda ending: np.load([f for f in written if f.endswith(ending)][0]),
                           best_model.MOMENT_HEADS[bool(best_model.GAUSS)][0], "post" if is_post else "prior")
            print(line)
            logging.debug("%s (%s)", line, written)
    if forecast_steps:
        t_out = best_model.horizon_times(int(forecast_steps))
        parts = {}
        for b in val_b:
            d = batch_to_device(b, device, family)
            for name, moments in best_model.forecast_moments(is_post=True, num_samples=num_samples, times_out=t_out, **d).items():
                for kind, val in zip(("mean", "sd"), moments):
                    parts.setdefault("%s_post_forecast_%s.npy" % (name, kind), []).append(val)
        written = best_model._save_arrays(out_dir, [(f, torch.cat(v, 0)) for f, v in parts.items()] + [("forecast_times.npy", t_out)])
        logging.debug("forecast moments: %s", written)
    if forecast_summary:
        t_out = best_model.horizon_times(int(forecast_steps))
        since = float(torch.as_tensor(best_model.times, dtype=torch.float32).reshape(-1)[-1])
        written = best_model.save_forecast_summary(out_dir, (batch_to_device(b, device, family) for b in val_b), True, int(forecast_summary), t_out,
                                                   since=since, thresholds=summary_thresholds, sense=summary_sense)
        for n in best_model.MOMENT_HEADS[bool(best_model.GAUSS)]:
            line = best_model.summary_line(np.load([f for f in written if f.endswith("summary_%s_post_forecast_mean.npy" % n)][0]), n,
                                           summary_thresholds is not None, name="forecast_summary")
            print(line)
            logging.debug("%s", line)
        logging.debug("forecast summary: %s", written)
    return var_model, best_model, best_epoch


def real_batches(config, family: str, data_dir: str):
    """(train_batches, val_batches, times or None) read from the reference's data files with the reference's transforms and splits
    (training_cvs.py:168-190, training_challenge.py:226-246); each an iterable of host batch dicts re-read every epoch."""
    from . import data as D
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if family == "cvs":
        tf = D.create_transforms(config.norm, D._torch_load(os.path.join(data_dir, "data_norm_params.pkl")))
        tr = D.CVSDataset(data_dir, "train", config.seq_len, False, tf)
        va = D.CVSDataset(data_dir, "val", config.seq_len, False, tf)
        te = D.CVSDataset(data_dir, "test", config.seq_len, False, tf)
    elif family == "challenge":
        pair = D.build_challenge_datasets(os.path.join(data_dir, "data.pkl"), config.seed, config.folds, config.split)
        tf = D.create_transforms(config.norm, pair.data_norm_params)
        tr, va = D.ChallengeDataset(pair.train, transforms=tf), D.ChallengeDataset(pair.test, transforms=tf)
    else:   # proc: observations are already [C, T]; the (non-uniform) time grid comes with the data
        tr, va, times = D.build_proc_datasets(data_dir, config.seed, config.folds, config.split, getattr(config, "heldout", None))
        config.seq_len = int(times.numel())
        return (D.BatchFeeder(tr, config.mini_batch_size, dev, shuffle=True, seed=config.seed),
                D.BatchFeeder(va, config.mini_batch_size, dev), times)
    class _AsBCT:
        """The datasets yield [B, T, C]; the models take the [B, C, T] permuted VIEW of it (training_cvs.py:25: no copy)."""

        def __init__(self, feeder):
            self.feeder = feeder

        def __len__(self):
            return len(self.feeder)

        def __iter__(self):
            for b in self.feeder:
                b["observations"] = b["observations"].permute(0, 2, 1)
                yield b

    out = (_AsBCT(D.BatchFeeder(tr, config.mini_batch_size, dev, shuffle=True, seed=config.seed)),
           _AsBCT(D.BatchFeeder(va, config.mini_batch_size, dev)), None)
    if family == "cvs":
        out = out + (_AsBCT(D.BatchFeeder(te, config.mini_batch_size, dev)),)
    return out


def build_parser():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batches-per-epoch", type=int, default=7)
    ap.add_argument("--data-dir", default=None, help="directory with the reference's data files (default: synthetic batches)")
    ap.add_argument("--fused-stats", action="store_true", help="per-epoch statistics: one engine call per batch, one read-back per pass")
    ap.add_argument("--sample-moments", action="store_true",
                    help="after training: mean and sd of config.num_samples reconstructions per curve (save_recon_moments), posterior and prior")
    ap.add_argument("--test-bounds", type=int, default=0, metavar="K",
                    help="after training: per-trajectory -ELBO, importance-weighted bound, ESS and NLL of the best model from K posterior draws over "
                         "the validation loader (save_trajectory_bounds: bounds_post.npy)")
    ap.add_argument("--label-evidence", type=int, default=0, metavar="K",
                    help="after training: the best model's own label posterior p(u | x) over the family's default hypotheses from K posterior draws "
                         "over the validation loader (save_label_evidence: evidence_*.npy) and its agreement with the subjects' labels, one line")
    ap.add_argument("--refine-steps", type=int, default=0, metavar="J",
                    help="after training: the best model's posterior refined per subject over the validation loader, J Adam steps on (loc, log "
                         "scale) against the subject's own -ELBO (save_refined_posterior: refined_*.npy), and the mean -ELBO before and after, one line")
    ap.add_argument("--refine-draws", type=int, default=8, metavar="K", help="draws per subject of --refine-steps (fixed for the whole refinement)")
    ap.add_argument("--waic", type=int, default=0, metavar="K",
                    help="after training: the best model's pointwise predictive density over the validation loader from K posterior draws "
                         "(save_pointwise_density: pointwise_*_post.npy, waic_post.npy) and its WAIC -- elpd_waic with its standard error, p_waic, "
                         "the share of points with p_waic > 0.4 -- one line")
    ap.add_argument("--loo", type=int, default=0, metavar="K",
                    help="after training: the best model's PSIS leave-one-out over the validation loader from K posterior draws "
                         "(save_pointwise_loo: pointwise_{elpd_loo,khat}_post.npy, loo_post.npy) -- elpd_loo with its standard error, p_loo, "
                         "the shares of points with khat > 0.7 and > 0.5 -- one line")
    ap.add_argument("--attribution", type=int, default=0, metavar="K",
                    help="after training: the best model's latent attribution over the validation loader from K pick-freeze draws, posterior and "
                         "prior (save_latent_attribution: attribution_*.npy, attribution_blocks.txt) -- per latent block, the mean total and "
                         "first-order variance index of the curves, one line per side")
    ap.add_argument("--curve-summary", type=int, default=0, metavar="K",
                    help="after training: the best model's curve summaries over the validation loader from K draws, posterior and prior "
                         "(save_curve_summary: summary_*.npy) -- per channel of the central curve, the mean peak, time to peak and AUC and, with "
                         "--summary-thresholds, P(cross) and the mean first crossing time, one line per side")
    ap.add_argument("--summary-thresholds", type=lambda v: [float(x) for x in v.split(",")], default=None, metavar="a,b,c[,d]",
                    help="one level per channel for --curve-summary (default: none; the threshold entries are then NaN)")
    ap.add_argument("--summary-sense", choices=("above", "below"), default="above",
                    help="which side of --summary-thresholds counts as beyond (default: above)")
    ap.add_argument("--intervention-summary", type=int, default=0, metavar="K",
                    help="after training: the best model's counterfactual summaries over the validation loader from K paired posterior draws on "
                         "the family's default hypotheses (save_intervention_summary: summary_<curve>_{factual,cf,effect}_*.npy) -- per hypothesis "
                         "and channel of the central curve, the mean paired effect on the peak and the AUC and, with --summary-thresholds / "
                         "--summary-sense, the change of P(cross), one line per hypothesis")
    ap.add_argument("--sample-quantiles", type=int, default=0, metavar="K",
                    help="after training: the best model's sample quantiles of every head curve over the validation loader from K draws, posterior "
                         "and prior (save_recon_quantiles: <curve>_<post|prior>_sample_quantiles.npy, sample_quantile_levels.npy) -- the mean band "
                         "width and the share of observation points inside the band, one line per side")
    ap.add_argument("--quantile-levels", type=lambda v: [float(x) for x in v.split(",")], default=[0.025, 0.975], metavar="a,b,...",
                    help="the levels of --sample-quantiles, 1 to 8 values in [0, 1] (default: 0.025,0.975)")
    ap.add_argument("--mechanism", type=int, default=0, metavar="K",
                    help="after training: the best model's mechanism curves over the validation loader from K draws, posterior and prior "
                         "(save_mechanism_moments: mechanism_<name>_<post|prior>_{mean,sd}.npy) -- per state component, the time-averaged mean "
                         "production, degradation and set point, one line per side")
    ap.add_argument("--joint-band", type=int, default=0, metavar="K",
                    help="after training: the best model's simultaneous (sup-t) credible bands over the validation loader from K draws, posterior "
                         "and prior (save_simultaneous_band: <curve>_<post|prior>_band_{mean,sd,crit,pointwise_joint,obs_dev}.npy, band_levels.npy) "
                         "-- the mean critical value beside the pointwise z, the share of draws wholly inside the pointwise band and the share of "
                         "observations wholly inside the simultaneous band, one line per side")
    ap.add_argument("--band-levels", type=lambda v: [float(x) for x in v.split(",")], default=[0.95], metavar="a,b,...",
                    help="the levels of --joint-band, 1 to 8 values in (0, 1] (default: 0.95)")
    ap.add_argument("--forecast-steps", type=int, default=0, metavar="N",
                    help="after training: the best model's posterior curves over the validation loader on the training grid extended by N steps, mean "
                         "and sd of config.num_samples draws (forecast_moments: <curve>_post_forecast_{mean,sd}.npy, forecast_times.npy)")
    ap.add_argument("--forecast-summary", type=int, default=0, metavar="K",
                    help="after training (needs --forecast-steps N > 0): the best model's forecast summaries over the validation loader from K "
                         "posterior draws on the extended grid, taken from the last training time on (save_forecast_summary: "
                         "summary_<curve>_post_forecast_{mean,sd}.npy) -- per channel of every head curve, the mean future peak and, with "
                         "--summary-thresholds / --summary-sense, P(cross) and the mean first crossing time, one line per curve")
    ap.add_argument("--cohort-curves", action="store_true",
                    help="after training: per-condition mean / sd curves, mean observations and the evaluation notebooks' l1_error on the first "
                         "test batch, posterior and prior (save_cohort_moments)")
    ap.add_argument("--calibration", action="store_true",
                    help="after training: quantile coverage against the nominal levels, band coverage, crossing share and pinball loss of the best "
                         "model over the validation loader, posterior and prior (save_calibration: calibration_*.npy)")
    return ap


def main(family: str, load_config, model_cls, model_cls_gauss, argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.forecast_summary and a.forecast_steps <= 0:
        ap.error("--forecast-summary needs --forecast-steps N > 0 (the horizon to summarise)")
    config = load_config()
    config.num_epochs = a.epochs
    os.makedirs("results_%s" % config.model, exist_ok=True)
    logging.basicConfig(filename="results_%s/model.log" % config.model, filemode="w", level=logging.DEBUG)
    kw = {"fused_stats": a.fused_stats}
    if a.sample_moments:
        kw["sample_moments"] = True
    if a.test_bounds:
        kw["test_bounds"] = a.test_bounds
    if a.label_evidence:
        kw["label_evidence"] = a.label_evidence
    if a.refine_steps:
        kw["refine_steps"], kw["refine_draws"] = a.refine_steps, a.refine_draws
    if a.waic:
        kw["waic"] = a.waic
    if a.loo:
        kw["loo"] = a.loo
    if a.attribution:
        kw["attribution"] = a.attribution
    if a.curve_summary:
        kw["curve_summary"], kw["summary_thresholds"], kw["summary_sense"] = a.curve_summary, a.summary_thresholds, a.summary_sense
    if a.intervention_summary:
        kw["intervention_summary"], kw["summary_thresholds"], kw["summary_sense"] = a.intervention_summary, a.summary_thresholds, a.summary_sense
    if a.sample_quantiles:
        kw["sample_quantiles"], kw["quantile_levels"] = a.sample_quantiles, a.quantile_levels
    if a.mechanism:
        kw["mechanism"] = a.mechanism
    if a.joint_band:
        kw["joint_band"], kw["band_levels"] = a.joint_band, a.band_levels
    if a.forecast_steps:
        kw["forecast_steps"] = a.forecast_steps
    if a.forecast_summary:
        kw["forecast_summary"], kw["summary_thresholds"], kw["summary_sense"] = a.forecast_summary, a.summary_thresholds, a.summary_sense
    if a.cohort_curves:
        kw["cohort_curves"] = True
    if a.calibration:
        kw["calibration"] = True
    if a.data_dir:
        got = real_batches(config, family, a.data_dir)
        kw["train_batches"], kw["val_batches"], kw["times"] = got[:3]
        if len(got) > 3:
            kw["test_batches"] = got[3]
    train(config, family, model_cls, model_cls_gauss, a.batches_per_epoch, **kw)
