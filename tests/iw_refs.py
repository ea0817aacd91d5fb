"""fp64 numpy restatement of the importance-weighted bound's device arithmetic (include/mst_hip.h: mst_iw_fold, mst_iw_finish), the
inputs of the kernel-level GPU test, and the bounds that test uses. Nothing here touches a GPU or the library.

state [B, 6] = {m, s, s2, sum_lw, n, n_bad};  out [B, 4] = {log_px, elbo, ess, n};  acc [6] = {sum log_px, sum elbo, sum ess, sum n,
pieces counted, pieces invalid}.

MUTANTS are deliberate mistakes in the reference; tests/test_iw_cpu.py checks that each of them leaves the bounds below, i.e. that the
GPU test would see the same mistake in the kernel."""
import numpy as np

M, S, S2, SUM_LW, N, N_BAD = range(6)
MUTANTS = ("no_log_sigma", "swap_z_eps", "no_s2_rescale", "no_log_n")

# Bounds of the kernel-level comparison. fp64 rounding: a log-weight is a sum of <= 3 * 260 + 1 terms, each rounded to 1.1e-16 relative,
# the exp / log of the recurrence a few ulp each; 1e-10 * (1 + sum |terms|) and 1e-9 relative leave three orders of margin.
ABS_TOL = 1e-10   # m, sum_lw, log_px (and elbo): times (1 + sum of |terms| of the sample's log-weights)
REL_TOL = 1e-9    # s, s2, ess

KERNEL_SHAPES = ((1, 1), (3, 5), (5, 64), (64, 256), (7, 260))  # (B, Z)
KERNEL_DRAWS = (1, 2, 9)


def log_weight(eps, sigma, z, recon, recon_scale, mutant=None):
    """lw [B] = -recon_scale * recon + sum_d (0.5 eps^2 - 0.5 z^2 + log|sigma|), fp64 on the fp32 inputs widened; also the sum of the
    absolute values of its terms (what the comparison's absolute bound scales with)"""
    e, sg, zz = (np.asarray(a, np.float32).astype(np.float64) for a in (eps, sigma, z))
    r = np.asarray(recon, np.float32).astype(np.float64)
    if mutant == "swap_z_eps":
        e, zz = zz, e
    with np.errstate(divide="ignore", invalid="ignore"):
        logs = np.zeros_like(sg) if mutant == "no_log_sigma" else np.log(np.abs(sg))
        terms = 0.5 * e * e - 0.5 * zz * zz + logs
        lw = -recon_scale * r + terms.sum(1)
        mag = np.abs(recon_scale * r) + (0.5 * e * e + 0.5 * zz * zz + np.abs(logs)).sum(1)
    return lw, mag


def fold_lw(state, lw, mutant=None):
    """one draw's log-weights [B] folded into a copy of state: the online update of mst_iw_fold, sample by sample"""
    st = np.array(state, np.float64, copy=True)
    for b, w in enumerate(np.asarray(lw, np.float64)):
        if not np.isfinite(w):
            st[b, N_BAD] += 1.0
            continue
        if st[b, N] == 0.0:
            st[b, M], st[b, S], st[b, S2] = w, 1.0, 1.0
        elif w > st[b, M]:
            d = st[b, M] - w
            st[b, S] = st[b, S] * np.exp(d) + 1.0
            st[b, S2] = (st[b, S2] if mutant == "no_s2_rescale" else st[b, S2] * np.exp(2.0 * d)) + 1.0
            st[b, M] = w
        else:
            r = np.exp(w - st[b, M])
            st[b, S] += r
            st[b, S2] += r * r
        st[b, SUM_LW] += w
        st[b, N] += 1.0
    return st


def fold(state, eps, sigma, z, recon, recon_scale, mutant=None):
    return fold_lw(state, log_weight(eps, sigma, z, recon, recon_scale, mutant)[0], mutant)


def finish(state, acc=None, mutant=None):
    """(out [B, 4], acc [6]) of mst_iw_finish; acc (optional) is added to, in ascending sample order"""
    st = np.asarray(state, np.float64)
    out = np.full((st.shape[0], 4), np.nan)
    acc = np.zeros(6) if acc is None else np.array(acc, np.float64, copy=True)
    add = np.zeros(6)
    for b in range(st.shape[0]):
        m, s, s2, sum_lw, n, n_bad = st[b]
        out[b, 3] = n
        if n > 0 and not n_bad > 0:
            out[b, 0] = m + np.log(s) - (0.0 if mutant == "no_log_n" else np.log(n))
            out[b, 1] = sum_lw / n
            out[b, 2] = s * s / s2
            add[:4] += out[b]
            add[4] += 1.0
        else:
            add[5] += 1.0
    return out, acc + add


def logsumexp_bound(lws):
    """the two-pass statement the recurrence is checked against: lws [K] finite log-weights of ONE sample ->
    (log_px = logsumexp - log K, elbo = mean, ess = (sum w)^2 / sum w^2 with w = exp(lw - max))"""
    lws = np.asarray(lws, np.float64)
    mx = lws.max()
    w = np.exp(lws - mx)
    return mx + np.log(w.sum()) - np.log(len(lws)), lws.mean(), w.sum() ** 2 / (w * w).sum()


# ---------------------------------------------------------------------------------------------- inputs of the kernel-level GPU test
SPECIALS = ("asc800", "desc800", "sigma0", "nan_eps", "inf_recon")  # what samples 0.. of a case are, as far as B allows


def special_rows(B):
    """sample index -> what is special about it. A batch of one stays plain; larger ones give their first rows to the specials"""
    return {} if B < 2 else {b: SPECIALS[b] for b in range(min(B, len(SPECIALS)))}


def kernel_case(B, Z, draws, seed=0):
    """K draws of real-range inputs as fp32 arrays: eps ~ N(0, 1), sigma in +-(0.4, 2.2) (a raw linear output: either sign), z = mu +
    eps sigma, a mean reconstruction loss around 0.1 with recon_scale 4096. Sample 0's log-weights arrive 800 nats apart in ascending
    order, sample 1's in descending order (through recon); in the draw `bad_draw` sample 2 has a sigma_d == 0, sample 3 a NaN eps and
    sample 4 an infinite recon — each must end invalid. Returns dict(eps, sigma, z [K, B, Z], recon [K, B], recon_scale, bad_draw)"""
    rng = np.random.default_rng([B, Z, draws, seed, 20270])
    scale = 4096.0
    mu = rng.standard_normal((B, Z))
    sg = rng.uniform(0.4, 2.2, (B, Z)) * np.where(rng.random((B, Z)) < 0.3, -1.0, 1.0)
    eps = rng.standard_normal((draws, B, Z)).astype(np.float32)
    sigma = np.broadcast_to(sg.astype(np.float32), (draws, B, Z)).copy()
    z = (mu[None].astype(np.float32) + eps * sigma).astype(np.float32)
    recon = rng.uniform(0.05, 0.15, (draws, B)).astype(np.float32)
    bad_draw = 0 if draws == 1 else 1
    for b, what in special_rows(B).items():
        k = np.arange(draws)
        if what == "asc800":
            recon[:, b] = (0.1 + (draws - 1 - k) * 800.0 / scale).astype(np.float32)   # recon falls: lw rises by 800 per draw
        elif what == "desc800":
            recon[:, b] = (0.1 + k * 800.0 / scale).astype(np.float32)
        elif what == "sigma0":
            sigma[bad_draw, b, Z // 2] = 0.0
        elif what == "nan_eps":
            eps[bad_draw, b, Z - 1] = np.nan
        elif what == "inf_recon":
            recon[bad_draw, b] = np.inf
    return dict(eps=eps, sigma=sigma, z=z, recon=recon, recon_scale=scale, bad_draw=bad_draw)


def fold_case(case, mutant=None):
    """-> (state after every draw of the case, sum over the draws of the |terms| of each sample's log-weights [B])"""
    K, B = case["recon"].shape
    st, mag = np.zeros((B, 6)), np.zeros(B)
    for k in range(K):
        lw, m = log_weight(case["eps"][k], case["sigma"][k], case["z"][k], case["recon"][k], case["recon_scale"], mutant)
        st = fold_lw(st, lw, mutant)
        mag += np.where(np.isfinite(m), m, 0.0)
    return st, mag


def compare(state, out, want_state, want_out, mag):
    """the kernel-level bounds: every out-of-tolerance quantity as a string (empty list: all within)"""
    bad = []
    state, out = np.asarray(state, np.float64), np.asarray(out, np.float64)
    tol = ABS_TOL * (1.0 + mag)
    valid = ~np.isnan(want_out[:, 0])
    if not np.array_equal(np.isnan(out[:, :3]), np.isnan(want_out[:, :3])):
        bad.append(f"validity: rows {np.flatnonzero(np.isnan(out[:, 0])).tolist()} are NaN, expected {np.flatnonzero(~valid).tolist()}")
    if not (np.array_equal(state[:, N], want_state[:, N]) and np.array_equal(state[:, N_BAD], want_state[:, N_BAD]) and
            np.array_equal(out[:, 3], want_out[:, 3])):
        bad.append(f"counts: n {state[:, N].tolist()} n_bad {state[:, N_BAD].tolist()}")
    seen = want_state[:, N] > 0
    for name, got, want, rows in (("m", state[:, M], want_state[:, M], seen), ("sum_lw", state[:, SUM_LW], want_state[:, SUM_LW], seen),
                                  ("log_px", out[:, 0], want_out[:, 0], valid), ("elbo", out[:, 1], want_out[:, 1], valid)):
        err = np.abs(got - want)[rows]
        if err.size and not (err <= tol[rows]).all():
            bad.append(f"{name}: error {err.max():.3g} against the bound {tol[rows][err.argmax()]:.3g}")
    for name, got, want, rows in (("s", state[:, S], want_state[:, S], seen), ("s2", state[:, S2], want_state[:, S2], seen),
                                  ("ess", out[:, 2], want_out[:, 2], valid)):
        with np.errstate(divide="ignore", invalid="ignore"):  # (rows outside `rows` may hold zeros and NaNs)
            err = (np.abs(got - want) / np.abs(want))[rows]
        if err.size and not (err <= REL_TOL).all():
            bad.append(f"{name}: relative error {err.max():.3g} > {REL_TOL:g}")
    return bad
