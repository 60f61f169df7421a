"""Double-precision numpy restatement of the correlation-structure metrics (osteosarcoma_diffusionmodel_amd/validation.py,
csrc/corr.hip), the cohorts the tests share and a numpy stand-in for ``DeviceKernels`` that the CPU tests drive the host code with."""
import functools

import numpy as np
import torch

STAT_KEYS = ("pairs", "sum_abs", "sum_sq", "max_abs", "strong_pairs", "strong_agree", "strong_sum_abs")
SUMMARY_KEYS = ["corr_mean_abs_diff", "corr_rms_diff", "corr_max_abs_diff", "corr_frobenius_diff", "corr_pairs", "corr_constant_columns",
                "corr_strong_pairs", "corr_strong_sign_agreement", "corr_strong_mean_abs_diff"]
FRECHET_KEYS = ["frechet_distance", "frechet_mean_term", "frechet_cov_term"]


def gram64(x, center=None):
    """(mu, G): double column means and sum_r (x_r - c)(x_r - c)^T in double; c = mu unless a centre is given."""
    a = np.asarray(x, dtype=np.float64)
    mu = a.mean(0)
    z = a - (mu if center is None else np.asarray(center, dtype=np.float64))
    return mu, z.T @ z


def corr_of_gram(G):
    """(r, live): r = G_ij / sqrt(G_ii G_jj) in double, NaN / inf where a column is constant; live marks G_ii > 0."""
    d = np.diag(G).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = G / np.sqrt(np.outer(d, d))
    return r, d > 0


def pair_masks(D, bounds, live):
    """Boolean [D, D] masks of the counted pairs (i < j, both columns live), one per block pair a <= b in row-major order."""
    iu = np.triu(np.ones((D, D), dtype=bool), 1) & live[:, None] & live[None, :]
    blk = np.searchsorted(np.asarray(bounds), np.arange(D), side="right") - 1
    nb = len(bounds) - 1
    return [iu & (blk[:, None] == a) & (blk[None, :] == b) for a in range(nb) for b in range(a, nb)]


def compare_stats(G_real, G_synth, bounds, strong, skip=None):
    """The dictionary of ``DeviceKernels.corr_compare`` from two double Gram matrices, by the definitions; ``skip``: a boolean
    [D, D] mask of pairs left out of the strong-pair counts (and of nothing else)."""
    D = G_real.shape[0]
    rr, live_r = corr_of_gram(G_real)
    rs, live_s = corr_of_gram(G_synth)
    live = live_r & live_s
    out = {k: [] for k in STAT_KEYS}
    for m in pair_masks(D, bounds, live):
        d = rs[m] - rr[m]
        st = np.abs(rr[m]) >= strong
        cnt = st if skip is None else st & ~skip[m]
        out["pairs"].append(int(m.sum()))
        out["sum_abs"].append(float(np.abs(d).sum()))
        out["sum_sq"].append(float((d * d).sum()))
        out["max_abs"].append(float(np.abs(d).max(initial=0.0)))
        out["strong_pairs"].append(int(cnt.sum()))
        out["strong_agree"].append(int((cnt & (np.sign(rs[m]) == np.sign(rr[m]))).sum()))
        out["strong_sum_abs"].append(float(np.abs(d[st]).sum()))
    res = {k: np.array(v, dtype=np.int64 if k in ("pairs", "strong_pairs", "strong_agree") else np.float64) for k, v in out.items()}
    res["constant_columns"] = int((~live).sum())
    return res


def summary_oracle(stats, names):
    """corr_summary restated from the definitions."""
    pairs, strong, agree = int(stats["pairs"].sum()), int(stats["strong_pairs"].sum()), int(stats["strong_agree"].sum())
    nan = float("nan")
    out = {"corr_mean_abs_diff": stats["sum_abs"].sum() / pairs if pairs else nan,
           "corr_rms_diff": np.sqrt(stats["sum_sq"].sum() / pairs) if pairs else nan,
           "corr_max_abs_diff": stats["max_abs"].max() if pairs else nan,
           "corr_frobenius_diff": np.sqrt(2.0 * stats["sum_sq"].sum()),
           "corr_pairs": pairs, "corr_constant_columns": stats["constant_columns"], "corr_strong_pairs": strong,
           "corr_strong_sign_agreement": agree / strong if strong else nan,
           "corr_strong_mean_abs_diff": stats["strong_sum_abs"].sum() / strong if strong else nan}
    if len(names) > 1:
        p = 0
        for a in range(len(names)):
            for b in range(a, len(names)):
                out[f"corr_mean_abs_diff_{names[a]}_{names[b]}"] = stats["sum_abs"][p] / stats["pairs"][p] if stats["pairs"][p] else nan
                p += 1
    return out


def frechet_oracle(mu1, S1, mu2, S2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum sqrt(eig(S1 S2)): the eigenvalues of the (non-symmetric) product are those of
    S1^(1/2) S2 S1^(1/2) -- real and non-negative up to rounding."""
    lam = np.linalg.eigvals(np.asarray(S1, dtype=np.float64) @ np.asarray(S2, dtype=np.float64))
    root = np.sqrt(np.clip(lam.real, 0.0, None)).sum()
    d = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    return float(d @ d + np.trace(S1) + np.trace(S2) - 2.0 * root)


@functools.lru_cache(maxsize=None)
def cohorts(n_real, n_synth, D, seed=0):
    """Two fp32 cohorts with a spread of correlations: a rank-4 factor model plus unit noise, every seventh column thresholded to
    0/1, the synthetic cohort's first half mixed with 0.3 x its second half, and a last column of mean 100 and sd 1.  Cached and
    shared between tests: copy before changing a value."""
    rs = np.random.default_rng(1000003 * seed + 7919 * n_real + 31 * n_synth + D)
    W = rs.standard_normal((4, D))
    out = []
    for which, n in enumerate((n_real, n_synth)):
        x = rs.standard_normal((n, 4)) @ W + rs.standard_normal((n, D))
        if which == 1 and D >= 2:
            x[:, :D // 2] += 0.3 * x[:, D - D // 2:]
        x[:, ::7] = (x[:, ::7] > 0.5).astype(np.float64)
        x[:, -1] = 100.0 + rs.standard_normal(n)
        out.append(x.astype(np.float32))
    return tuple(out)


class NumpyKernels:
    """``column_sums``, ``centered_gram`` and ``corr_compare`` with the semantics of validation.DeviceKernels, in double on the host.
    ``centered_gram`` subtracts the centre ROUNDED TO fp32, as the device kernel does."""

    @staticmethod
    def column_sums(t):
        return t.double().numpy().sum(0)

    @staticmethod
    def centered_gram(t, center):
        c = np.asarray(center, dtype=np.float32).astype(np.float64)
        z = t.double().numpy() - c
        return torch.from_numpy(z.T @ z)

    @staticmethod
    def corr_compare(g_real, g_synth, bounds, strong):
        return compare_stats(g_real.numpy(), g_synth.numpy(), list(bounds), strong)
