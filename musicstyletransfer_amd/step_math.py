"""Host statements of the formulas the device evaluates and the checks of the options that switch them on. numpy and
math only: importable without torch or the kernel library."""
import math

import numpy as np


def roll_scores(tp, pred, pos, cells):
    """the piano-roll counts of ParamStore.read_metrics (a cell is predicted where its logit is > 0) as scores: precision = tp / pred,
    recall = tp / pos, f1 = 2 tp / (pred + pos), cell_acc = (cells - pred - pos + 2 tp) / cells; NaN where a denominator is 0"""
    nan = float("nan")
    return dict(precision=tp / pred if pred else nan, recall=tp / pos if pos else nan,
                f1=2 * tp / (pred + pos) if pred + pos else nan,
                cell_acc=(cells - pred - pos + 2 * tp) / cells if cells else nan)


def latent_scores(acc, threshold=0.01):
    """the per-class, per-dimension sums of ParamStore.read_metrics' 'lat_stats' (fp64 [C, 5, Z], planes {n, sum mu, sum mu^2,
    sum sigma^2, sum kl_d}: mst_latent_dim_stats) as scores. Per dimension d, pooled over the classes: n, m = sum mu / n,
    V = sum mu^2 / n - m^2 (the variance of the posterior mean over the data).
      active_units  number of dimensions with V > threshold (Burda et al.'s 0.01)
      kl_dims       [Z] mean KL of each dimension, sum kl_d / n
      kl_dim_max    the largest of kl_dims
      kl_dims_used  number of dimensions with mean KL > threshold
      sigma_rms     sqrt(mean over d of sum sigma^2 / n)
      class_leak    max over the active dimensions of eta^2_d = sum_c (n_c / n) (m_cd - m_d)^2 / V_d, the share of a dimension's variance
                    that lies BETWEEN the classes (0: z says nothing about the class; 1: the class alone decides mu_d). NaN without an
                    active dimension, or when fewer than two classes have samples.
    A dimension with n == 0 has NaN entries and is not active (kl_dim_max and sigma_rms are taken over the dimensions with samples)."""
    acc = np.asarray(acc, np.float64)
    if acc.ndim != 3 or acc.shape[1] != 5:
        raise ValueError(f"latent_scores takes [C, 5, Z] sums, not {acc.shape}")
    nan = float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        n_c = acc[:, 0]                                   # [C, Z]
        n, s_mu, s_mu2, s_s2, s_kl = acc.sum(0)           # [Z] each
        m = s_mu / n
        var = s_mu2 / n - m * m
        kl_dims = s_kl / n
        active = var > threshold                          # (NaN compares false)
        m_c = acc[:, 1] / n_c                             # [C, Z]; NaN for a class without samples: its weight below is 0
        between = np.where(n_c > 0, n_c / n * (m_c - m) ** 2, 0.0).sum(0)
        eta2 = np.minimum(between / var, 1.0)             # (between <= V; the two are rounded apart)
    seen = n > 0
    classes_seen = int((n_c.sum(1) > 0).sum())
    leak = float(eta2[active].max()) if active.any() and classes_seen >= 2 else nan
    return dict(active_units=int(active.sum()), kl_dims=kl_dims, kl_dim_max=float(kl_dims[seen].max()) if seen.any() else nan,
                kl_dims_used=int((kl_dims > threshold).sum()),
                sigma_rms=float(np.sqrt((s_s2[seen] / n[seen]).mean())) if seen.any() else nan, class_leak=leak)


def class_mmd_score(acc):
    """the three running sums of ParamStore.read_metrics' 'class_mmd_acc' (mst_class_mmd: sum of L over the launches whose L was
    finite, those launches, the launches whose L was not finite) as the reported figures: class_mmd = sum / count, the mean penalty
    L = sum_c (n_c / n) MMD^2(q_c, q_pooled) per counted batch (NaN when none was counted), and class_mmd_bad, the other launches"""
    acc = np.asarray(acc, np.float64).reshape(-1)
    if acc.size != 3:
        raise ValueError(f"class_mmd_score takes the three sums of mst_class_mmd, not {acc.size} values")
    return dict(class_mmd=float(acc[0] / acc[1]) if acc[1] > 0 else float("nan"), class_mmd_bad=int(acc[2]))


def check_class_mmd(class_mmd=0.0, class_mmd_s2=None):
    """class_mmd: the penalty's multiplier lambda, 0 (off) or positive and finite; class_mmd_s2: the kernel's bandwidth s2, None or 0
    (the latent width Z) or positive and finite; raises ValueError otherwise (a NaN too)"""
    if not (0 <= class_mmd < float("inf")):
        raise ValueError(f"class_mmd must be 0 (off) or a positive finite multiplier, not {class_mmd!r}")
    if class_mmd_s2 is not None and not (0 <= class_mmd_s2 < float("inf")):
        raise ValueError(f"class_mmd_s2 (class_mmd_bandwidth) must be 0 (the latent width) or a positive finite bandwidth, not {class_mmd_s2!r}")


def iw_scores(acc, cells):
    """the six running sums of IWBound (ops.IW_ACC: sum log_px, sum elbo, sum ess, sum n, pieces counted, pieces invalid — mst_iw_finish)
    as the reported figures, stated once. cells: cells per piece (T * P for a piano-roll, T for a token sequence). Nats per piece:
      iw_nll            -sum log_px / pieces     the importance-weighted bound on -log p(x)
      iw_elbo_nll       -sum elbo / pieces       the same draws' mean log-weight: the ELBO in nats
      iw_gap            iw_elbo_nll - iw_nll     >= 0 (Jensen); near 0: the posterior is tight, or the decoder ignores z
      iw_ess            sum ess / pieces         effective sample size of the weights, between 1 and K
      iw_bits_per_cell  iw_nll / (cells ln 2)
      iw_invalid        pieces with a draw that was not finite (in none of the sums)
    NaN where no piece was counted."""
    acc = np.asarray(acc, np.float64).reshape(-1)
    if acc.size != 6:
        raise ValueError(f"iw_scores takes the six sums of mst_iw_finish, not {acc.size} values")
    if not cells > 0:
        raise ValueError(f"cells per piece must be positive, not {cells!r}")
    pieces, nan = acc[4], float("nan")
    nll = -acc[0] / pieces if pieces > 0 else nan
    elbo_nll = -acc[1] / pieces if pieces > 0 else nan
    return dict(iw_nll=float(nll), iw_elbo_nll=float(elbo_nll), iw_gap=float(elbo_nll - nll),
                iw_ess=float(acc[2] / pieces) if pieces > 0 else nan, iw_bits_per_cell=float(nll / (cells * math.log(2.0))),
                iw_invalid=int(acc[5]))


def check_iw(samples):
    """samples: K of the importance-weighted bound, an integer >= 1 (1: the one-sample ELBO); raises ValueError otherwise (a NaN, a
    bool and a fraction too)"""
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
        raise ValueError(f"iw_samples must be an integer >= 1, not {samples!r}")


def check_schedule(kl_warmup_steps=0, kl_cycle_steps=0, kl_free_bits=0.0, lr_warmup_steps=0):
    """the combinations of training-schedule settings that mean something; raises ValueError otherwise"""
    for name, val in (("kl_warmup_steps", kl_warmup_steps), ("kl_cycle_steps", kl_cycle_steps), ("lr_warmup_steps", lr_warmup_steps)):
        if int(val) != val or val < 0:
            raise ValueError(f"{name} must be a non-negative integer, not {val!r}")
    if not kl_free_bits >= 0:
        raise ValueError(f"kl_free_bits must be >= 0 nats per sample, not {kl_free_bits!r}")
    if kl_cycle_steps > 0 and kl_warmup_steps == 0:
        raise ValueError("kl_cycle_steps restarts the KL warm-up: it needs kl_warmup_steps > 0")
    if kl_cycle_steps > 0 and kl_warmup_steps > kl_cycle_steps:
        raise ValueError(f"kl_warmup_steps ({kl_warmup_steps}) must not exceed kl_cycle_steps ({kl_cycle_steps})")


def check_clip(clip_global_norm=0.0):
    """clip_global_norm: 0 (off) or a positive finite bound on the gradient's global L2 norm; raises ValueError otherwise"""
    if not (0 <= clip_global_norm < float("inf")):
        raise ValueError(f"clip_global_norm must be 0 (off) or a positive finite norm, not {clip_global_norm!r}")


def check_input_dropout(d_input_dropout=0.0):
    """d_input_dropout: probability in [0, 1] that a decoder input position is dropped in a training step (0: off, 1: every position);
    raises ValueError otherwise (a NaN too)"""
    if not (0 <= d_input_dropout <= 1):
        raise ValueError(f"d_input_dropout must lie in [0, 1], not {d_input_dropout!r}")


def clip_scale(norm, max_norm):
    """the factor c global-norm clipping applies to a gradient of L2 norm `norm` — gluon.utils.clip_global_norm's rule as the device
    evaluates it (mst_adam_flat's clipping group), stated once for the host in np.float32 arithmetic: c = max_norm / (norm + 1e-8), and 1 unless
    that is below 1"""
    c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-8))
    return c if c < np.float32(1) else np.float32(1)


def check_ema(ema_decay=0.0):
    """ema_decay: 0 (off) or the decay of the weights' exponential moving average, in (0, 1); raises ValueError otherwise (a NaN too)"""
    if not (0 <= ema_decay < 1):
        raise ValueError(f"ema_decay must be 0 (off) or lie in (0, 1), not {ema_decay!r}")


def ema_decay_at(t, decay):
    """d_t, the decay the average applies at training step t (Adam's step count after the step's increment, 1-based) — the rule as the
    device evaluates it (mst_adam_flat's averaging group), stated once for the host in np.float32 arithmetic: min(decay, (1 + t) / (10 + t)), the usual
    warm-up, so that the first steps do not average in the initial weights"""
    tf = np.float32(t)
    d = (np.float32(1) + tf) / (np.float32(10) + tf)
    return min(np.float32(decay), d)


def ema_update(e, w_new, d):
    """the average after a step: fl(fl(d * e) + fl((1 - d) * w_new)) in np.float32 — two rounded products and one rounded sum, in this
    order and never fused, which is what mst_adam_flat computes for mst_adam_args.ema (include/mst_hip.h) bit for bit. e, w_new: fp32 arrays (or scalars)"""
    d = np.float32(d)
    omd = np.float32(1) - d
    a = d * np.asarray(e, np.float32)
    b = omd * np.asarray(w_new, np.float32)
    return a + b


def schedule_values(t, kl_weight=1.0, kl_warmup_steps=0, kl_cycle_steps=0, lr_warmup_steps=0):
    """(beta_t, f_lr) of training step t (Adam's step count after the step's increment, 1-based) — the formulas the device evaluates
    (step_begin.hpp), stated once for the host. Double arithmetic; beta_t is rounded once, to fp32, and returned as that value:
        f_lr   = min(1, t / W_lr) if W_lr > 0 else 1                 the step runs at lr * f_lr
        u      = ((t - 1) mod C) + 1 if C > 0 else t                 position in the current KL cycle
        beta_t = fp32(fp32(kl_weight) * (min(1, u / W_b) if W_b > 0 else 1))"""
    f_lr = min(1.0, t / lr_warmup_steps) if lr_warmup_steps > 0 else 1.0
    u = (t - 1) % kl_cycle_steps + 1 if kl_cycle_steps > 0 else t
    ramp = min(1.0, u / kl_warmup_steps) if kl_warmup_steps > 0 else 1.0
    return float(np.float32(float(np.float32(kl_weight)) * ramp)), f_lr
