"""fp64 references of mst_token_step's cuts (no GPU, no library): the kept set of a row of stored 16-bit logits under a temperature, a
top-k and a nucleus cut, twice — as cuts on the stored value (the header's wording) and as a brute-force walk down the sorted row —
and the generator of the test cases, which fits top_p to the row so that the reference's kept set is the only admissible answer.

The rules (include/mst_hip.h), for one row over columns 0..V-1:
  x_j = logit_j / tau in fp32;  s = softmax(x): the sampling distribution;  p = softmax(logit): the model's own
  top-k: c_k = the k-th largest stored logit with multiplicity; logit_j >= c_k survives (top_k = 0 or >= V: all)
  top-p: among the survivors, c_p = the largest stored value c with mass_s{logit_j >= c} >= top_p * mass_s{survivors};
         logit_j >= c_p is kept (top_p = 1: all survivors)."""
import numpy as np
import torch

SAMPLE_V = (1, 5, 64, 65, 127, 293, 2051)  # tests/test_decode_kernels_gpu.py: the chunk geometries of one wave per sequence
DTYPES = (torch.bfloat16, torch.float16)
TAUS = (0.5, 1.0, 2.0)
TARGETS = (0.1, 0.5, 0.9)


def delta(V):
    """worst case of an fp32 sum of V terms, plus expf: the relative error a mass formed in fp32 can carry"""
    return (V + 8) * 2.0 ** -23


def _dists(row16, tau):
    """(stored values fp64, s, p) of a 1-D 16-bit tensor"""
    assert row16.dtype in DTYPES and row16.dim() == 1
    v = row16.double().numpy()
    x = (row16.float() / torch.tensor(float(tau), dtype=torch.float32)).double().numpy()  # the division is the kernel's: fp32
    s = np.exp(x - x.max())
    p = np.exp(v - v.max())
    return v, s / s.sum(), p / p.sum()


def token_filter_ref(row16, tau, top_k, top_p):
    """-> (kept mask bool [V], s fp64 [V], p fp64 [V]) by the cut rules; top_p is taken as the fp32 number the kernel is handed"""
    v, s, p = _dists(row16, tau)
    V = len(v)
    top_p = float(np.float32(top_p))
    assert top_k >= 0 and 0.0 < top_p <= 1.0
    if top_k == 0 or top_k >= V:
        surv = np.ones(V, bool)
    else:
        c_k = np.sort(v)[::-1][top_k - 1]
        surv = v >= c_k
    if top_p >= 1.0:
        return surv, s, p
    need = top_p * s[surv].sum()
    c_p = None
    for c in np.unique(v[surv]):  # ascending: the last one that still holds the mass is the largest
        if s[surv & (v >= c)].sum() >= need:
            c_p = c
    assert c_p is not None
    return surv & (v >= c_p), s, p


def token_filter_brute(row16, tau, top_k, top_p):
    """the same kept set the long way: sort, walk down whole tie groups, accumulate"""
    v, s, _ = _dists(row16, tau)
    V = len(v)
    top_p = float(np.float32(top_p))
    order = sorted(range(V), key=lambda j: -v[j])
    groups, j = [], 0
    while j < V:
        g = [order[j]]
        while j + len(g) < V and v[order[j + len(g)]] == v[g[0]]:
            g.append(order[j + len(g)])
        groups.append(g)
        j += len(g)
    k = V if (top_k == 0 or top_k >= V) else top_k
    surv_groups, n = [], 0
    for g in groups:  # groups until k tokens are in: the one that crosses k comes whole
        if n >= k:
            break
        surv_groups.append(g)
        n += len(g)
    kept = np.zeros(V, bool)
    if top_p >= 1.0:
        for g in surv_groups:
            kept[g] = True
        return kept
    total = sum(s[j] for g in surv_groups for j in g)
    surv_idx = [j for g in surv_groups for j in g]
    for m in range(1, len(surv_groups) + 1):  # the smallest number of groups whose mass reaches top_p of the survivors'
        idx = [j for g in surv_groups[:m] for j in g]
        mask = np.zeros(V, bool)
        mask[idx] = True
        # (the mass is summed as token_filter_ref sums it — a boolean mask over the row in column order — so the two forms
        # compare the very same fp64 number with the bound and cannot disagree by an ulp)
        surv_mask = np.zeros(V, bool)
        surv_mask[surv_idx] = True
        if s[mask].sum() >= top_p * s[surv_mask].sum():
            kept[idx] = True
            return kept
    raise AssertionError("the survivors' whole mass is below top_p of itself")


def make_row(V, dtype, seed):
    """randn(V) * 3 rounded to the dtype"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, generator=g) * 3.0).to(dtype)


def plant_ties(row16, k, width=9):
    """the value of rank k placed on `width` columns around rank k (ranks k - width // 2 .. ): a tie group that straddles the top-k cut"""
    V = row16.numel()
    order = torch.argsort(row16.float(), descending=True, stable=True)
    lo = max(0, k - 1 - width // 2)
    hi = min(V, lo + width)
    out = row16.clone()
    out[order[lo:hi]] = row16[order[min(k - 1, V - 1)]]
    return out


def cum_masses(row16, tau, top_k):
    """cumulative masses (fractions of the survivors' mass, fp64) of the descending distinct stored values among the top-k survivors"""
    v, s, _ = _dists(row16, tau)
    surv, _, _ = token_filter_ref(row16, tau, top_k, 1.0)
    vals = np.unique(v[surv])[::-1]
    total = s[surv].sum()
    return np.array([s[surv & (v >= c)].sum() / total for c in vals])


def fit_top_p(row16, tau, top_k, target):
    """top_p fitted to the row: of the steps of the cumulative mass (0 -> cum[0] -> cum[1] ...) larger than 4 delta (+ an fp32 ulp of
    top_p, for rounding the midpoint), the one whose midpoint is nearest the target; top_p = that midpoint as an fp32. Then every
    cumulative mass is at least 2 delta away from top_p: no fp32 rounding of a mass can move the cut.
    -> (top_p, number of distinct values kept)"""
    V = row16.numel()
    cum = cum_masses(row16, tau, top_k)
    edges = np.concatenate([[0.0], cum])
    best = None
    for g in range(len(cum)):
        size = edges[g + 1] - edges[g]
        if size <= 4 * delta(V) + 2.0 ** -22:
            continue
        mid = float(np.float32(0.5 * (edges[g] + edges[g + 1])))
        if not 0.0 < mid < 1.0:
            continue
        if best is None or abs(mid - target) < abs(best[0] - target):
            best = (mid, g + 1)
    assert best is not None, "no step of the cumulative mass is wide enough"
    return best


def margin(row16, tau, top_k, top_p):
    """distance of top_p to the nearest cumulative mass (0 included), in units of delta(V)"""
    cum = np.concatenate([[0.0], cum_masses(row16, tau, top_k)])
    return float(np.abs(cum - float(np.float32(top_p))).min() / delta(row16.numel()))
