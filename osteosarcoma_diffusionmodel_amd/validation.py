"""Validation metrics on MI355X -- host-side mirror of the reference's utils/validation.py.
Same class, method names and result keys as ``BiologicalValidator`` including ``validate_all``; everything that
scales with the number of patients runs in libosdiff.so (``osd_val_*``): RBF-MMD, per-feature two-sample KS, pathway
coherence, the mutation-expression sign check, mutation frequencies and the joint mutation counts behind the
chi-square co-occurrence test and the mutual-exclusivity check.  Beyond the reference: ``marginal_fidelity``, the KS distance, the
Wasserstein-1 distance and the out-of-range share of EVERY feature (``osd_val_marginals``), among the other added checks below.

Host-side by design, as SURVEY section 8f-1 prescribes: p-values and chi-square statistics from the exact device counts
(``scipy.stats``), and the Wasserstein distance on 10 principal components (``sklearn`` PCA + ``scipy``, :256-269),
which the reference itself computes that way -- by default; ``statistical_tests(..., pca="device")`` takes it from
``pca.DevicePCA`` without downloading a cohort, and ``embedding_fidelity`` builds the ``pca_*`` checks on the same fit.

Multi-GPU (BASELINE config 5): ``BiologicalValidator(config, sharded=True)`` under an initialised
``torch.distributed`` treats every *synthetic* argument as this rank's row shard (the real cohort is small and
replicated).  Accumulators are summed over ranks (``parallel.ShardComm``), the all-pairs synthetic Gram block walks
the shards by broadcast, the <= 100 KS columns are gathered and split by feature.  Every rank returns the same
numbers as one process on the concatenated rows.
"""
from __future__ import annotations

import ctypes as C
import logging
import weakref
from math import gcd
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import cluster as CL
from . import diffexp as DE
from . import enrichment as EN
from . import pathways as PW
from . import pca as PC
from . import survival as SV
from . import utility as U
from .cluster import subtype_summary      # noqa: F401  (the subtype_* figures: pure NumPy, documented there)
from .parallel import ShardComm

logger = logging.getLogger(__name__)

PATHWAY_METHODS = PW.METHODS        # the method numbers of osd_val_pathway_scores


def _dev(a, device) -> torch.Tensor:
    """fp32 contiguous [n, d] tensor on the device from numpy / DataFrame / tensor."""
    if hasattr(a, "values") and not isinstance(a, torch.Tensor):
        a = a.values
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(device=device, dtype=torch.float32).contiguous()


class DeviceFrame:
    """The few DataFrame operations BiologicalValidator touches (``.columns``, ``.values``, column selection, a column's
    ``.mean()``) over a tensor that already lives on the device: the validator's inputs at BASELINE config 5's size (10^5-10^6
    generated patients x 2000 features per GPU) never visit the host as a pandas object."""

    def __init__(self, values: torch.Tensor, columns):
        import pandas as pd
        self.values = values
        self.columns = columns if isinstance(columns, pd.Index) else pd.Index(list(columns))

    @property
    def shape(self):
        return tuple(self.values.shape)

    def __getitem__(self, key):
        if isinstance(key, str):
            return self.values[:, self.columns.get_loc(key)]          # a device vector: .mean() works as on a Series
        key = list(key)
        if len(key) == len(self.columns) and all(a == b for a, b in zip(key, self.columns)):
            return self
        idx = torch.as_tensor(self.columns.get_indexer(key), device=self.values.device)
        return DeviceFrame(self.values.index_select(1, idx), key)


def _host(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a.values if hasattr(a, "values") else a)


def _ks_pvalue(n1: int, n2: int, dmax: int, dmin: int):
    """(statistic, p-value) from the integer extremes, following scipy.stats.ks_2samp(method='auto'):
    exact when max(n1, n2) <= 10000, Smirnov's asymptotic formula otherwise (a scalar per feature)."""
    from scipy.stats import distributions
    from scipy.stats._stats_py import _attempt_exact_2kssamp
    d = max(dmax, -dmin, 0) / (float(n1) * float(n2))
    if max(n1, n2) <= 10000:
        ok, d2, prob = _attempt_exact_2kssamp(n1, n2, gcd(n1, n2), d, "two-sided")
        if ok:
            return float(d2), float(np.clip(prob, 0, 1))
    m, n = sorted([float(n1), float(n2)], reverse=True)
    return float(d), float(np.clip(distributions.kstwo.sf(d, np.round(m * n / (m + n))), 0, 1))


def _ks_pvalues(n1: int, n2: int, dmax, dmin):
    """_ks_pvalue over all features.  Above 10 000 samples ks_2samp(method='auto') takes Smirnov's asymptotic formula: ONE
    vectorised scipy call for the whole statistic vector (same values as the per-feature calls -- kstwo.sf is elementwise -- without
    100 trips through rv_continuous' argument checking: 0.8 s -> 10 ms at 100 features); the exact branch stays per feature."""
    dmax, dmin = np.asarray(dmax, dtype=np.int64), np.asarray(dmin, dtype=np.int64)
    if max(n1, n2) <= 10000:
        res = [_ks_pvalue(n1, n2, int(a), int(b)) for a, b in zip(dmax, dmin)]
        return np.array([d for d, _ in res]), np.array([p for _, p in res])
    from scipy.stats import distributions
    d = np.maximum(np.maximum(dmax, -dmin), 0) / (float(n1) * float(n2))
    m, n = sorted([float(n1), float(n2)], reverse=True)
    return d.astype(np.float64), np.clip(distributions.kstwo.sf(d, np.round(m * n / (m + n))), 0, 1).astype(np.float64)


def _chi2_pairs(n: int, gram: np.ndarray) -> np.ndarray:
    """chi2 of scipy.stats.chi2_contingency(pd.crosstab(a_i, a_j)) (utils/validation.py:98-108) for every pair i < j of 0/1 columns,
    row-major pair order, from the joint counts gram[i][j] = sum_r a_i a_j -- the closed form of what scipy does for a 2 x 2 table
    (expected = outer(margins) / n, Yates' correction min(0.5, |expected - observed|) toward the expected value, Pearson sum), and
    0.0 when a column is constant (crosstab then has a single row or column: zero degrees of freedom).  Same values as the
    per-pair scipy calls (tests/test_oracle_golden.py), 2 x 1225 tables in one numpy expression instead of 0.26 s of calls."""
    g = np.rint(np.asarray(gram, dtype=np.float64))
    k = g.shape[0]
    iu, ju = np.triu_indices(k, 1)
    n1, n2, n11 = np.diag(g)[iu], np.diag(g)[ju], g[iu, ju]
    obs = np.stack([n - n1 - n2 + n11, n2 - n11, n1 - n11, n11], axis=-1).reshape(-1, 2, 2)      # [[00, 01], [10, 11]]
    rows, cols = obs.sum(2), obs.sum(1)
    exp = rows[:, :, None] * cols[:, None, :] / float(n)
    live = (rows > 0).all(1) & (cols > 0).all(1)
    diff = exp - obs
    adj = obs + np.minimum(0.5, np.abs(diff)) * np.sign(diff)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = (adj - exp) ** 2 / exp
    return np.where(live, np.where(live[:, None, None], terms, 0.0).sum((1, 2)), 0.0)


def _cox_plan_destroy(handle: int) -> None:
    L.lib().osd_val_cox_plan_destroy(C.c_void_p(handle))


class CoxPlan:
    """What ``osd_val_cox_eval`` needs of a cohort's (time, event) columns, made once per fit by ``DeviceKernels.cox_plan``: the
    library's plan handle, its row count and the stream its calls run on.  ``close()`` destroys the plan (again: nothing); a
    finalizer does it for a plan that was never closed."""

    def __init__(self, handle: int, rows: int, stream: Optional[int] = None):
        self.handle, self.rows, self.stream = C.c_void_p(handle), int(rows), stream
        self._finalizer = weakref.finalize(self, _cox_plan_destroy, handle)

    @property
    def closed(self) -> bool:
        return not self._finalizer.alive

    def close(self) -> None:
        self._finalizer()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DeviceKernels:
    """The per-shard partial results, each one libosdiff.so call on device tensors."""

    def __init__(self, device: torch.device):
        self.device = device
        self.index = device.index if device.index is not None else torch.cuda.current_device()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def rbf_sum(self, a: torch.Tensor, b: torch.Tensor, gamma: float) -> float:
        out = C.c_double()
        L.check(L.lib().osd_val_rbf_sum(self._stream(), self.index, L.ptr(a), a.shape[0], L.ptr(b), b.shape[0], a.shape[1], float(gamma),
                                        C.byref(out)))
        return float(out.value)

    def nearest(self, q: torch.Tensor, r: torch.Tensor, exclude: Optional[torch.Tensor] = None):
        """(d2 float32 [nq], idx int32 [nq]) device tensors: each row of q against the rows of r, row ``exclude[i]`` skipped."""
        _same_features(q, r)
        nq = q.shape[0]
        d2 = torch.empty(nq, dtype=torch.float32, device=q.device)
        idx = torch.empty(nq, dtype=torch.int32, device=q.device)
        exclude = _exclude(exclude, q)
        L.check(L.lib().osd_val_nearest(self._stream(), self.index, L.ptr(q), nq, L.ptr(r), r.shape[0], q.shape[1], L.ptr(exclude),
                                        L.ptr(d2), L.ptr(idx)))
        return d2, idx

    def knn(self, q: torch.Tensor, r: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None):
        """(d2 float32 [nq, k], idx int32 [nq, k]) device tensors: the k nearest rows of r for each row of q in ascending order of
        the recomputed distance, row ``exclude[i]`` skipped; (+inf, -1) where r has fewer than k candidates.  1 <= k <= 16."""
        _same_features(q, r)
        nq = q.shape[0]
        d2 = torch.empty((nq, max(int(k), 0)), dtype=torch.float32, device=q.device)
        idx = torch.empty((nq, max(int(k), 0)), dtype=torch.int32, device=q.device)
        exclude = _exclude(exclude, q)
        L.check(L.lib().osd_val_knn(self._stream(), self.index, L.ptr(q), nq, L.ptr(r), r.shape[0], q.shape[1], int(k), L.ptr(exclude),
                                    L.ptr(d2), L.ptr(idx)))
        return d2, idx

    def ball_counts(self, q: torch.Tensor, r: torch.Tensor, r2_ref: Optional[torch.Tensor] = None,
                    r2_query: Optional[torch.Tensor] = None):
        """(in_ref, in_query) int32 [nq] device tensors, None where the radius is None: for each row of q the number of rows of r
        within the r row's squared radius ``r2_ref[f]``, and within the q row's own squared radius ``r2_query[p]`` (``<=``)."""
        _same_features(q, r)
        nq, nr = q.shape[0], r.shape[0]
        outs = []
        for name, rad, n in (("r2_ref", r2_ref, nr), ("r2_query", r2_query, nq)):
            if rad is not None:
                rad = rad.to(device=q.device, dtype=torch.float32).contiguous()
                if rad.shape != (n,):
                    raise ValueError(f"{name} must hold one squared radius per row ({n})")
            outs.append((rad, None if rad is None else torch.empty(nq, dtype=torch.int32, device=q.device)))
        (rr, in_ref), (rq, in_query) = outs
        L.check(L.lib().osd_val_ball_counts(self._stream(), self.index, L.ptr(q), nq, L.ptr(r), nr, q.shape[1], L.ptr(rr), L.ptr(rq),
                                            L.ptr(in_ref), L.ptr(in_query)))
        return in_ref, in_query

    def ks_extremes(self, real: torch.Tensor, synth: torch.Tensor, nf: int):
        dmax, dmin = (C.c_int64 * nf)(), (C.c_int64 * nf)()
        L.check(L.lib().osd_val_ks_extremes(self._stream(), self.index, L.ptr(real), real.shape[0], L.ptr(synth), synth.shape[0],
                                            real.shape[1], nf, dmax, dmin))
        return np.array(dmax[:], dtype=np.int64), np.array(dmin[:], dtype=np.int64)

    def marginals(self, real: torch.Tensor, synth: torch.Tensor, chunk_cols: int = 0, phases: bool = False) -> Dict[str, np.ndarray]:
        """``osd_val_marginals`` on two fp32 device tensors [n1, D] and [n2, D] (column-slice views are read in place): per feature
        ``ks_dmax``, ``ks_dmin`` (int64, the exact extremes ``ks_extremes`` returns), ``w1`` (float64, the Wasserstein-1 distance by
        quantile coupling) and ``below``, ``above`` (int64, synthetic values outside the real column's range), numpy arrays [D].
        ``chunk_cols``: columns sorted at a time (0: the library's choice); the results do not depend on it.  ``phases=True`` adds
        ``phase_ms``, the device milliseconds of (gather, sort, statistics).  The same inputs give the same bits."""
        real, synth = _rows_view(real), _rows_view(synth)
        _same_features(real, synth)
        (n1, D), n2 = real.shape, synth.shape[0]
        outs = [np.zeros(D, dtype=dt) for dt in (np.int64, np.int64, np.float64, np.int64, np.int64)]
        args = [self._stream(), self.index, L.ptr(real), n1, max(int(real.stride(0)), D), L.ptr(synth), n2, max(int(synth.stride(0)), D), D,
                int(chunk_cols)] + [C.c_void_p(o.ctypes.data) for o in outs]
        if phases:
            ms = (C.c_double * 3)()
            L.check(L.lib().osd_val_marginals_timed(*args, ms))
        else:
            L.check(L.lib().osd_val_marginals(*args))
        res = dict(zip(MARGINAL_FIELDS, outs))
        if phases:
            res["phase_ms"] = np.array(ms[:])
        return res

    def group_ranks(self, t: torch.Tensor, labels: torch.Tensor, center=None, chunk_cols: int = 0, phases: bool = False):
        """``osd_val_group_ranks`` on the fp32 device tensor t [rows, D] (a column-slice view is read in place) and the int32 labels
        [rows] -- 1 a case, 0 a control, anything else ignored: a dictionary of numpy arrays, per feature ``u2`` (int64 [D], twice the
        Mann-Whitney U of the cases over the controls, ties counted 1/2), ``ties`` (int64 [D], the sum of t^3 - t over the tie groups
        of the pooled column) and ``sum``, ``sumsq`` (float64 [2, D]: cases, controls; of x - c and its square), plus the group
        sizes ``na`` and ``nb``.  ``center``: D values rounded to fp32, or None for 0.  ``chunk_cols``: columns sorted at a time (0:
        the library's choice).  ``phases=True`` adds ``phase_ms``, the device milliseconds of (gather, sort, statistics).  The same
        bits at every ``chunk_cols``, on every call and for every order of the rows.  An empty group is a ValueError."""
        t = _rows_view(t)
        rows, D = t.shape
        labels = labels.to(device=t.device, dtype=torch.int32).contiguous()
        if labels.shape != (rows,):
            raise ValueError(f"labels must hold one label per row ({rows})")
        c = None if center is None else _f32(center, t.device, (D,), "center")
        u2, ties = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
        s, q = np.zeros((2, D), dtype=np.float64), np.zeros((2, D), dtype=np.float64)
        na, nb = C.c_int64(), C.c_int64()
        args = [self._stream(), self.index, L.ptr(t), rows, max(int(t.stride(0)), D), D, L.ptr(labels), L.ptr(c), int(chunk_cols)]
        args += [C.c_void_p(o.ctypes.data) for o in (u2, ties, s, q)] + [C.c_void_p(C.addressof(na)), C.c_void_p(C.addressof(nb))]
        if phases:
            ms = (C.c_double * 3)()
            L.check(L.lib().osd_val_group_ranks_timed(*args, ms))
        else:
            L.check(L.lib().osd_val_group_ranks(*args))
        res = {"u2": u2, "ties": ties, "sum": s, "sumsq": q, "na": int(na.value), "nb": int(nb.value)}
        if phases:
            res["phase_ms"] = np.array(ms[:])
        return res

    def gsea(self, weights, set_positions, permutations: int, seed: int = 0, perm_chunk: int = 0, phases: bool = False):
        """``osd_val_gsea``: the running-sum extremes of S gene sets under the identity and ``permutations`` gene-label permutations.
        ``weights``: float64 [D], the weight of every position of the ranked list; ``set_positions``: per set an integer array of
        its members' ranked positions, in any order.  A dictionary of numpy arrays: ``es_pos`` and ``es_neg`` (float64
        [permutations + 1, S], row 0 observed) and ``lead`` (int32 [S, 2]: the first hit number, counted along the set's sorted
        hits, that attains the observed maximum and minimum).  ``perm_chunk``: permutations per workspace chunk (0: the library's
        choice); ``phases=True`` adds ``phase_ms``, the device milliseconds of (keys and ranks, hit sort, scan).  The same bits at
        every ``perm_chunk`` and on every call.  A ValueError for what the library refuses: D outside [2, 32768], no set, a set
        with no member, more than 1024 or all D positions, a position outside [0, D) or repeated in a set, a weight that is
        negative, not finite or above 1e100, a negative ``permutations`` or ``perm_chunk``."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 1:
            raise ValueError("weights must be a vector")
        sets = [np.ascontiguousarray(np.asarray(m).reshape(-1), dtype=np.int64) for m in set_positions]
        D, S, P = int(w.shape[0]), len(sets), int(permutations)
        if S < 1 or P < 0 or int(perm_chunk) < 0:
            raise ValueError("at least one set, permutations >= 0 and perm_chunk >= 0 are needed")
        if any(m.size and (m.min() < -2 ** 31 or m.max() >= 2 ** 31) for m in sets) or sum(m.size for m in sets) >= 2 ** 31:
            raise ValueError("set positions must fit 32 bits")
        offsets = np.zeros(S + 1, dtype=np.int32)
        offsets[1:] = np.cumsum([m.size for m in sets])
        flat = np.ascontiguousarray(np.concatenate(sets), dtype=np.int32) if offsets[-1] else np.zeros(1, dtype=np.int32)
        es_pos, es_neg = np.zeros((P + 1, S), dtype=np.float64), np.zeros((P + 1, S), dtype=np.float64)
        lead = np.zeros((S, 2), dtype=np.int32)
        args = [self._stream(), self.index, C.c_void_p(w.ctypes.data), D, C.c_void_p(offsets.ctypes.data), C.c_void_p(flat.ctypes.data),
                S, P, int(seed) & (2 ** 64 - 1), int(perm_chunk)] + [C.c_void_p(o.ctypes.data) for o in (es_pos, es_neg, lead)]
        if phases:
            ms = (C.c_float * 3)()
            L.check(L.lib().osd_val_gsea_timed(*args, ms))
        else:
            L.check(L.lib().osd_val_gsea(*args))
        res = {"es_pos": es_pos, "es_neg": es_neg, "lead": lead}
        if phases:
            res["phase_ms"] = np.array(ms[:], dtype=np.float64)
        return res

    def pathway_scores(self, t: torch.Tensor, sets, method: str = "mean", center=None, scale=None, rank_table=None,
                       row_chunk: int = 0, phases: bool = False):
        """``osd_val_pathway_scores`` on the fp32 device tensor t [rows, D] (a column-slice view is read in place): a float64 DEVICE
        tensor [rows, S], per row the score of every set -- ``sets``: per set an integer array of its distinct columns.  ``method``:
        ``mean`` (sum_j (x_j - c_j) s_j / m), ``zscore`` (the same sum / sqrt(m)) or ``ssgsea`` (the closed form over the row's
        mid-ranks; ``rank_table``: float64 [2 D + 1], ``pathways.rank_table(D, alpha)``).  ``center``, ``scale``: D values rounded to
        fp32, or None for 0 and for 1.  ``row_chunk``: rows per launch (0: the library's choice); ``phases=True`` returns
        (scores, phase_ms), the device milliseconds of (staging, scoring).  The same bits at every ``row_chunk`` and on every
        call.  A ValueError for what the library refuses: D outside [2, 32768], no set, a set with no member, more than 1024 or
        all D columns, a column outside [0, D) or repeated in a set, a negative ``row_chunk``, ``ssgsea`` without its table."""
        if method not in PATHWAY_METHODS:
            raise ValueError(f"method must be one of {PATHWAY_METHODS}, got {method!r}")
        t = _rows_view(t)
        rows, D = t.shape
        sets = [np.ascontiguousarray(np.asarray(m).reshape(-1), dtype=np.int64) for m in sets]
        S = len(sets)
        if S < 1 or int(row_chunk) < 0:
            raise ValueError("at least one set and row_chunk >= 0 are needed")
        if any(m.size and (m.min() < -2 ** 31 or m.max() >= 2 ** 31) for m in sets) or sum(m.size for m in sets) >= 2 ** 31:
            raise ValueError("set members must fit 32 bits")
        offsets = np.zeros(S + 1, dtype=np.int32)
        offsets[1:] = np.cumsum([m.size for m in sets])
        flat = np.ascontiguousarray(np.concatenate(sets), dtype=np.int32) if offsets[-1] else np.zeros(1, dtype=np.int32)
        c = None if center is None else _f32(center, t.device, (D,), "center")
        s = None if scale is None else _f32(scale, t.device, (D,), "scale")
        table = None
        if method == "ssgsea":
            if rank_table is None:
                raise ValueError("ssgsea needs rank_table, float64 [2 D + 1]")
            table = np.ascontiguousarray(rank_table, dtype=np.float64)
            if table.shape != (2 * D + 1,):
                raise ValueError(f"rank_table must have shape ({2 * D + 1},), got {table.shape}")
        out = torch.empty((rows, S), dtype=torch.float64, device=t.device)
        args = [self._stream(), self.index, L.ptr(t), rows, max(int(t.stride(0)), D), D, PATHWAY_METHODS.index(method), L.ptr(c), L.ptr(s),
                C.c_void_p(offsets.ctypes.data), C.c_void_p(flat.ctypes.data), S,
                C.c_void_p(0 if table is None else table.ctypes.data), int(row_chunk), L.ptr(out)]
        if phases:
            ms = (C.c_float * 2)()
            L.check(L.lib().osd_val_pathway_scores_timed(*args, ms))
            return out, np.array(ms[:], dtype=np.float64)
        L.check(L.lib().osd_val_pathway_scores(*args))
        return out

    def pathway_agreement(self, scores: torch.Tensor, block: torch.Tensor, mu, isd) -> Dict[str, np.ndarray]:
        """``osd_val_pathway_agreement``: ``scores`` a float64 device tensor [rows, S] (``pathway_scores``), ``block`` an fp32 device
        tensor [rows, >= S] (a column-slice view is read in place; its first S columns are used), ``mu`` and ``isd`` float64 [S].
        With z = (score - mu) * isd and g the block's value, over the rows where both are finite: ``sums`` float64 [S, 6] (sum z,
        sum g, sum z^2, sum g^2, sum z g, sum (g - z)^2) and ``used`` int64 [S], the number of those rows.  The same bits on every
        call."""
        if scores.dtype != torch.float64 or scores.dim() != 2 or not scores.is_contiguous() or scores.shape[0] < 1 or scores.shape[1] < 1:
            raise ValueError("scores must be a contiguous float64 [rows >= 1, S >= 1] tensor")
        rows, S = scores.shape
        block = _rows_view(block)
        if block.shape[0] != rows or block.shape[1] < S:
            raise ValueError(f"block must be [{rows}, >= {S}], got {tuple(block.shape)}")
        mu, isd = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(isd, dtype=np.float64)
        if mu.shape != (S,) or isd.shape != (S,):
            raise ValueError(f"mu and isd must hold one value per pathway ({S})")
        sums, used = np.zeros((S, 6), dtype=np.float64), np.zeros(S, dtype=np.int64)
        L.check(L.lib().osd_val_pathway_agreement(self._stream(), self.index, L.ptr(scores), rows, S, L.ptr(block),
                                                  max(int(block.stride(0)), int(block.shape[1])), C.c_void_p(mu.ctypes.data),
                                                  C.c_void_p(isd.ctypes.data), C.c_void_p(sums.ctypes.data), C.c_void_p(used.ctypes.data)))
        return {"sums": sums, "used": used}

    def col_moments(self, t: torch.Tensor, cols: Sequence[int]):
        g, arr = _col_array(cols)
        s, q = (C.c_double * g)(), (C.c_double * g)()
        L.check(L.lib().osd_val_col_moments(self._stream(), self.index, L.ptr(t), t.shape[0], t.shape[1], arr, g, s, q))
        return np.array(s[:]), np.array(q[:])

    def rowz_sq(self, t: torch.Tensor, cols: Sequence[int], mu: np.ndarray, isd: np.ndarray) -> float:
        g, arr = _col_array(cols)
        out = C.c_double()
        L.check(L.lib().osd_val_rowz_sq(self._stream(), self.index, L.ptr(t), t.shape[0], t.shape[1], arr, g, (C.c_double * g)(*mu),
                                        (C.c_double * g)(*isd), C.byref(out)))
        return float(out.value)

    def pearson_sums(self, t_a: torch.Tensor, col_a: int, t_b: torch.Tensor, col_b: int) -> np.ndarray:
        out = (C.c_double * 5)()
        L.check(L.lib().osd_val_pearson_sums(self._stream(), self.index, C.c_void_p(t_a.data_ptr() + 4 * col_a), t_a.shape[1],
                                             C.c_void_p(t_b.data_ptr() + 4 * col_b), t_b.shape[1], t_a.shape[0], out))
        return np.array(out[:])

    def column_sums(self, t: torch.Tensor) -> np.ndarray:
        out = (C.c_double * t.shape[1])()
        L.check(L.lib().osd_val_column_sums(self._stream(), self.index, L.ptr(t), t.shape[0], t.shape[1], t.shape[1], out))
        return np.array(out[:])

    def gram(self, t: torch.Tensor, cols: Sequence[int]) -> np.ndarray:
        g, arr = _col_array(cols)
        if g > 64:
            raise ValueError("at most 64 columns per Gram block")
        out = (C.c_double * (g * g))()
        L.check(L.lib().osd_val_gram(self._stream(), self.index, L.ptr(t), t.shape[0], t.shape[1], arr, g, out))
        return np.array(out[:]).reshape(g, g)

    def centered_gram(self, t: torch.Tensor, center) -> torch.Tensor:
        """float64 [D, D] DEVICE tensor G[i][j] = sum_r (t[r][i] - c[i]) (t[r][j] - c[j]) over all D columns of the fp32 device
        tensor t (``osd_val_centered_gram``: fp32 differences and products, double sums, exactly symmetric, the same bits on every
        call).  ``center``: D values, rounded to fp32 -- what the kernel subtracts.  A column-slice view is read in place."""
        t = _rows_view(t, "centered_gram needs a [rows >= 1, features >= 1] tensor")
        rows, D = t.shape
        c = np.ascontiguousarray(center, dtype=np.float32)
        if c.shape != (D,):
            raise ValueError(f"center must hold one value per column ({D})")
        g = torch.empty((D, D), dtype=torch.float64, device=t.device)
        L.check(L.lib().osd_val_centered_gram(self._stream(), self.index, L.ptr(t), rows, max(int(t.stride(0)), D), D,
                                              C.c_void_p(c.ctypes.data), L.ptr(g)))
        return g

    def corr_compare(self, g_real: torch.Tensor, g_synth: torch.Tensor, bounds: Sequence[int], strong: float) -> Dict[str, np.ndarray]:
        """The figures of ``osd_val_corr_compare`` for two float64 [D, D] device Gram matrices: ``constant_columns`` (an int) and,
        one entry per block pair a <= b in row-major order, ``pairs``, ``strong_pairs``, ``strong_agree`` (int64) and ``sum_abs``,
        ``sum_sq``, ``max_abs``, ``strong_sum_abs`` (float64).  ``bounds``: 0 = b_0 < ... < b_B = D."""
        D = g_real.shape[0]
        for g in (g_real, g_synth):
            if g.dtype != torch.float64 or tuple(g.shape) != (D, D) or not g.is_contiguous():
                raise ValueError("the Gram matrices must be contiguous float64 [D, D] tensors of the same size")
        nb = len(bounds) - 1
        if nb < 1:
            raise ValueError("at least one column block")
        arr = (C.c_int32 * (nb + 1))(*[int(b) for b in bounds])
        n_pairs = nb * (nb + 1) // 2
        out = (C.c_double * (1 + L.OSD_CORR_STATS * n_pairs))()
        L.check(L.lib().osd_val_corr_compare(self._stream(), self.index, L.ptr(g_real), L.ptr(g_synth), D, arr, nb, float(strong), out))
        return corr_stats_from_flat(np.array(out[:]))

    def col_centered_moments(self, t: torch.Tensor, center=None):
        """(sum, sumsq) float64 [D] numpy: per column of the fp32 device tensor t the sums of (x - c) and (x - c)^2 in double
        (``osd_val_col_centered_moments``; one pass, fixed order).  ``center``: D values rounded to fp32, or None for 0.  A
        column-slice view is read in place."""
        t = _rows_view(t)
        rows, D = t.shape
        c = None if center is None else _f32(center, t.device, (D,), "center")
        s, q = (C.c_double * D)(), (C.c_double * D)()
        L.check(L.lib().osd_val_col_centered_moments(self._stream(), self.index, L.ptr(t), rows, max(int(t.stride(0)), D), D, L.ptr(c), s, q))
        return np.array(s[:]), np.array(q[:])

    def glm_eval(self, x: torch.Tensor, center, scale, y, W, kinds: Sequence[int], row_weight=None, grad: bool = True,
                 scores: bool = False):
        """``osd_val_glm_eval`` on the fp32 device tensor x [rows, D] (a column-slice view is read in place): with
        u = (x - center) * scale and z = W[:, :D] u + W[:, D], returns ``(loss, grad, scores)`` -- loss float64 [K] numpy, the SUM
        over the rows of a_i l_k(y_ik, z_ik) (None without targets); grad float64 [K, D + 1] numpy, its gradient, bias last (None
        with ``grad=False``: the predictor); scores the float32 [rows, K] device tensor z (None unless ``scores=True``).
        ``center``, ``scale`` [D], ``W`` [K, D + 1], ``y`` [rows, K] and ``row_weight`` [rows] (None: 1) are rounded to fp32;
        ``kinds``: ``utility.LOGISTIC`` / ``utility.SQUARED`` per head, K <= 4.  Sums, not means, and no penalty: the results of
        several calls add up.  The same inputs give the same bits."""
        x = _rows_view(x)
        rows, D = x.shape
        K = len(kinds)
        center, scale = _f32(center, x.device, (D,), "center"), _f32(scale, x.device, (D,), "scale")
        W = _f32(W, x.device, (K, D + 1), "W")
        y = None if y is None else _f32(y, x.device, (rows, K), "y")
        a = None if row_weight is None else _f32(row_weight, x.device, (rows,), "row_weight")
        if y is None and grad:
            raise ValueError("a gradient needs targets")
        if y is None and not scores:
            raise ValueError("nothing to compute: no targets and no scores")
        arr = (C.c_int32 * max(K, 1))(*[int(v) for v in kinds])
        loss = (C.c_double * max(K, 1))() if y is not None else None
        g = torch.empty((K, D + 1), dtype=torch.float64, device=x.device) if grad else None
        z = torch.empty((rows, K), dtype=torch.float32, device=x.device) if scores else None
        L.check(L.lib().osd_val_glm_eval(self._stream(), self.index, L.ptr(x), rows, max(int(x.stride(0)), D), D, L.ptr(center),
                                         L.ptr(scale), L.ptr(y), K, L.ptr(a), L.ptr(W), K, arr, loss, L.ptr(g), L.ptr(z), K))
        return (None if loss is None else np.array(loss[:K])), (None if g is None else g.cpu().numpy()), z

    def label_sums(self, t: torch.Tensor, labels: torch.Tensor, K: int, value: Optional[torch.Tensor] = None):
        """``osd_val_label_sums`` on the fp32 device tensor t [rows, D] (a column-slice view is read in place) and the int32 labels
        [rows]: ``(sums, counts, value_sums)`` DEVICE tensors -- sums float64 [K, D], the column sums of the rows of each label;
        counts int64 [K]; value_sums float64 [K], the per-label sums of ``value`` [rows] (rounded to fp32), or None without one.  A
        row whose label lies outside [0, K) -- ``nearest``'s -1 included -- contributes to nothing.  Every addition is in double and
        in a fixed order: the same inputs give the same bits.  1 <= K <= 64, D <= 8192."""
        t = _rows_view(t)
        rows, D = t.shape
        K = int(K)
        labels = labels.to(device=t.device, dtype=torch.int32).contiguous()
        if labels.shape != (rows,):
            raise ValueError(f"labels must hold one label per row ({rows})")
        v = None if value is None else _f32(value, t.device, (rows,), "value")
        sums = torch.empty((max(K, 0), D), dtype=torch.float64, device=t.device)
        counts = torch.empty(max(K, 0), dtype=torch.int64, device=t.device)
        vs = None if v is None else torch.empty(max(K, 0), dtype=torch.float64, device=t.device)
        L.check(L.lib().osd_val_label_sums(self._stream(), self.index, L.ptr(t), rows, max(int(t.stride(0)), D), D, L.ptr(labels), K,
                                           L.ptr(v), L.ptr(sums), L.ptr(counts), L.ptr(vs)))
        return sums, counts, vs


    def cox_plan(self, time, event) -> CoxPlan:
        """``osd_val_cox_plan_create`` for a cohort's follow-up times and event flags (host arrays, one per row): the library sorts
        the rows by descending time, finds the tie groups and uploads them.  Non-finite times and flags other than 0 or 1 are a
        ValueError.  The plan belongs to this device and the current stream; ``close()`` it after the fit."""
        t = np.ascontiguousarray(np.asarray(time, dtype=np.float64).ravel())
        d = np.ascontiguousarray(np.asarray(event, dtype=np.float64).ravel())
        if t.shape != d.shape:
            raise ValueError("one event flag per time")
        h, stream = C.c_void_p(), self._stream()
        L.check(L.lib().osd_val_cox_plan_create(self.index, stream, t.ctypes.data, d.ctypes.data, t.size, C.byref(h)))
        return CoxPlan(h.value, t.size, stream.value)

    def cox_eval(self, x: torch.Tensor, center, scale, w, plan: CoxPlan, grad: bool = True, scores: bool = False):
        """``osd_val_cox_eval`` on the fp32 device tensor x [rows, D] (a column-slice view is read in place) and the plan of its
        rows: with u = (x - center) * scale and eta = w . u, returns ``(loss, grad, scores)`` -- loss the negative Breslow partial
        log-likelihood, a float SUM over the rows; grad float64 [D] numpy, its gradient (None with ``grad=False``); scores the
        float32 [rows] device tensor eta (None unless ``scores=True``).  ``center``, ``scale`` and ``w`` [D] are rounded to fp32.
        No penalty and no 1 / n: the host applies them.  The same inputs give the same bits.  The call runs on the stream the plan
        was made on; under another current stream that stream is waited for first, so the inputs are ready."""
        if plan.closed:
            raise ValueError("the plan has been closed")
        x = _rows_view(x)
        rows, D = x.shape
        center, scale, w = (_f32(v, x.device, (D,), name) for v, name in ((center, "center"), (scale, "scale"), (w, "w")))
        loss = C.c_double()
        g = torch.empty(D, dtype=torch.float64, device=x.device) if grad else None
        z = torch.empty(rows, dtype=torch.float32, device=x.device) if scores else None
        if self._stream().value != plan.stream:
            torch.cuda.current_stream(self.device).synchronize()
        L.check(L.lib().osd_val_cox_eval(plan.handle, L.ptr(x), rows, max(int(x.stride(0)), D), D, L.ptr(center), L.ptr(scale), L.ptr(w),
                                         C.byref(loss), L.ptr(g), L.ptr(z)))
        return float(loss.value), (None if g is None else g.cpu().numpy()), z

    def cox_score(self, x: torch.Tensor, center, scale, plan: CoxPlan, beta=None, bound=None, absmax: bool = False):
        """``osd_val_cox_score`` on the fp32 device tensor x [rows, D] (a column-slice view is read in place) and the plan of its
        rows: one Cox model per column, in double.  With u = (x - center) * scale, returns ``(loglik, score, info, absmax)``, float64
        [D] numpy each: every column's Breslow partial log-likelihood at its own ``beta[c]``, its derivative, minus its second
        derivative, and max_i |u_ic| (None unless ``absmax=True``).  ``beta`` [D] float64 (None: 0, a path without exp); ``bound``
        [D] float64, R_c >= max |u_ic|, shifts the exponent to beta u - |beta| R <= 0 (None: no shift); ``center`` and ``scale`` [D]
        are rounded to fp32.  A column with scale 0 gives exact zeros.  The same inputs give the same bits, and a column gives the
        same bits whatever other columns the call holds.  Runs on the plan's stream, as ``cox_eval`` does."""
        if plan.closed:
            raise ValueError("the plan has been closed")
        x = _rows_view(x)
        rows, D = x.shape
        center, scale = _f32(center, x.device, (D,), "center"), _f32(scale, x.device, (D,), "scale")

        def f64(v, name):
            if v is None:
                return None
            t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
            t = t.to(device=x.device, dtype=torch.float64).contiguous()
            if tuple(t.shape) != (D,):
                raise ValueError(f"{name} must have shape ({D},), got {tuple(t.shape)}")
            return t

        b, r = f64(beta, "beta"), f64(bound, "bound")
        out = torch.empty((4, D), dtype=torch.float64, device=x.device)
        if self._stream().value != plan.stream:
            torch.cuda.current_stream(self.device).synchronize()
        L.check(L.lib().osd_val_cox_score(plan.handle, L.ptr(x), rows, max(int(x.stride(0)), D), D, L.ptr(center), L.ptr(scale), L.ptr(b),
                                          L.ptr(r), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]) if absmax else None))
        host = out.cpu().numpy()
        return host[0], host[1], host[2], (host[3] if absmax else None)

    def col_moments64(self, t: torch.Tensor, center=None):
        """``col_centered_moments`` for a row shard that may be empty: (sum, sumsq) float64 [D] numpy of (x - c) and (x - c)^2 over
        the rows of the fp32 device tensor t [rows >= 0, D], exact zeros without rows.  The partial sums of row shards about one
        common centre add up, which is how ``pca.DevicePCA`` takes its float64 mean and sample sd."""
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError("a [rows, features >= 1] tensor is needed")
        if int(t.shape[0]) == 0:
            return np.zeros(int(t.shape[1])), np.zeros(int(t.shape[1]))
        return self.col_centered_moments(t, center)

    def _pca_args(self, x: torch.Tensor, center, scale, m, m_rows: int):
        """(x view, rows, D, l, center, scale, m) as ``osd_val_pca_*`` take them: float64 contiguous device tensors."""
        x = _rows_view(x)
        rows, D = x.shape

        def f64(v, shape, name):
            t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
            t = t.to(device=x.device, dtype=torch.float64).contiguous()
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
            return t

        if not hasattr(m, "shape") or len(m.shape) != 2:
            raise ValueError("the directions must be a [*, l] matrix")
        l = int(m.shape[1])
        return (x, rows, D, l, f64(center, (D,), "center"), None if scale is None else f64(scale, (D,), "scale"),
                f64(m, (D if m_rows < 0 else m_rows, l), "the direction matrix"))

    def pca_project(self, x: torch.Tensor, center, scale, V, norm2: bool = False):
        """``osd_val_pca_project`` on the fp32 device tensor x [rows, D] (a column-slice view is read in place): with
        u = ((double) x - center) * scale (``scale`` None: 1), returns ``(Z, norm2)`` DEVICE float64 tensors -- Z [rows, l] = u V
        and norm2 [rows] = sum_c u^2 (None unless ``norm2=True``).  ``center``, ``scale`` [D] and ``V`` [D, l] are float64 (numpy
        or tensors).  1 <= l <= 32, l <= D <= 32768.  Every sum is in double and in a fixed order: the same inputs give the same
        bits.  A tensor without rows gives empty results."""
        if x.dim() == 2 and int(x.shape[0]) == 0 and int(x.shape[1]) >= 1:
            l = int(V.shape[1])
            return (torch.empty((0, l), dtype=torch.float64, device=x.device),
                    torch.empty(0, dtype=torch.float64, device=x.device) if norm2 else None)
        x, rows, D, l, c, s, v = self._pca_args(x, center, scale, V, -1)
        z = torch.empty((rows, l), dtype=torch.float64, device=x.device)
        n2 = torch.empty(rows, dtype=torch.float64, device=x.device) if norm2 else None
        L.check(L.lib().osd_val_pca_project(self._stream(), self.index, L.ptr(x), rows, max(int(x.stride(0)), D), D, L.ptr(c), L.ptr(s),
                                            L.ptr(v), l, L.ptr(z), L.ptr(n2)))
        return z, n2

    def pca_backproject(self, x: torch.Tensor, center, scale, Z) -> torch.Tensor:
        """``osd_val_pca_backproject`` on the fp32 device tensor x [rows, D] (a column-slice view is read in place): the DEVICE
        float64 tensor W [D, l] = u^T Z with u as in ``pca_project`` and ``Z`` float64 [rows, l].  The same inputs give the same
        bits; the results of row shards add up.  A tensor without rows gives zeros."""
        if x.dim() == 2 and int(x.shape[0]) == 0 and int(x.shape[1]) >= 1:
            return torch.zeros((int(x.shape[1]), int(Z.shape[1])), dtype=torch.float64, device=x.device)
        x, rows, D, l, c, s, z = self._pca_args(x, center, scale, Z, int(x.shape[0]))
        w = torch.empty((D, l), dtype=torch.float64, device=x.device)
        L.check(L.lib().osd_val_pca_backproject(self._stream(), self.index, L.ptr(x), rows, max(int(x.stride(0)), D), D, L.ptr(c),
                                                L.ptr(s), L.ptr(z), l, L.ptr(w)))
        return w

    def concordance(self, time, event, risk):
        """``osd_val_concordance``: the exact pair counts ``(comparable, concordant, discordant, tied_risk)`` of
        ``survival.concordance_counts`` as Python integers.  The three columns [n] are rounded to fp32 and compared as such."""
        cols = []
        for v, name in ((time, "time"), (event, "event"), (risk, "risk")):
            v = v.reshape(-1) if isinstance(v, torch.Tensor) else np.asarray(v).ravel()
            cols.append(_f32(v, self.device, (int(v.shape[0]),), name))
        n = int(cols[0].shape[0])
        if any(int(c.shape[0]) != n for c in cols):
            raise ValueError("time, event and risk must have one value per row")
        out = (C.c_int64 * 4)()
        L.check(L.lib().osd_val_concordance(self._stream(), self.index, L.ptr(cols[0]), L.ptr(cols[1]), L.ptr(cols[2]), n, out))
        return tuple(int(v) for v in out)


def _same_features(q: torch.Tensor, r: torch.Tensor) -> None:
    if q.shape[1] != r.shape[1]:
        raise ValueError("q and r must have the same number of features")


def _exclude(exclude: Optional[torch.Tensor], q: torch.Tensor) -> Optional[torch.Tensor]:
    """``exclude`` as a contiguous int32 tensor on q's device, one index per row of q (None stays None)."""
    if exclude is not None:
        exclude = exclude.to(device=q.device, dtype=torch.int32).contiguous()
        if exclude.shape != (q.shape[0],):
            raise ValueError("exclude must hold one index per query row")
    return exclude


def _col_array(cols: Sequence[int]):
    """(g, ctypes int32 [g]): a column list as the library takes it."""
    return len(cols), (C.c_int32 * len(cols))(*cols)


def _rows_view(t: torch.Tensor, what: str = "a [rows >= 1, features >= 1] tensor is needed") -> torch.Tensor:
    """t as an fp32 [rows >= 1, D >= 1] tensor whose rows are contiguous (stride(1) == 1, stride(0) >= D): itself where it already is."""
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(what)
    if t.dtype != torch.float32 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.to(torch.float32).contiguous()
    return t


def _f32(a, device, shape, name: str) -> torch.Tensor:
    """a as a contiguous fp32 tensor of the given shape on the device."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


COV_SLAB_ROWS = 256       # OSD_COV_SLAB_ROWS of include/osdiff.h: rows one fp32 accumulator run of osd_val_centered_gram covers
_CORR_FIELDS = ("pairs", "sum_abs", "sum_sq", "max_abs", "strong_pairs", "strong_agree", "strong_sum_abs")
_CORR_INT_FIELDS = ("pairs", "strong_pairs", "strong_agree")


def corr_stats_from_flat(flat: np.ndarray) -> Dict[str, np.ndarray]:
    """osd_val_corr_compare's host array (1 + 7 figures per block pair) as the dictionary ``DeviceKernels.corr_compare`` returns."""
    flat = np.asarray(flat, dtype=np.float64)
    table = flat[1:].reshape(-1, L.OSD_CORR_STATS)
    out = {"constant_columns": int(round(flat[0]))}
    for i, name in enumerate(_CORR_FIELDS):
        out[name] = np.rint(table[:, i]).astype(np.int64) if name in _CORR_INT_FIELDS else table[:, i].copy()
    return out


# ---- combination of per-shard partials (pure host logic; the CPU tests drive it over gloo with numpy kernels) -----------
def sharded_mmd(comm: ShardComm, k, x, y_local, gamma: float) -> float:
    """utils/validation.py:273-298 with X replicated and Y row-sharded."""
    n = x.shape[0]
    m = int(comm.sum(y_local.shape[0])[0])
    sxx = k.rbf_sum(x, x, gamma)                       # one operand: the library runs the upper triangle only (csrc/validate.hip)
    sxy = float(comm.sum(k.rbf_sum(x, y_local, gamma))[0])
    # K_YY is symmetric: this shard against itself (triangular) + every unordered pair of shards once, weighted 2
    syy_local = k.rbf_sum(y_local, y_local, gamma)
    for other, weight in comm.ring_partners(y_local):
        syy_local += weight * k.rbf_sum(y_local, other, gamma)
    syy = float(comm.sum(syy_local)[0])
    v = sxx / (float(n) * n) + syy / (float(m) * m) - 2.0 * sxy / (float(n) * m)
    return float(np.sqrt(max(v, 0.0)))


def sharded_ks_extremes(comm: ShardComm, k, real, synth_local, nf: int):
    """Integer KS extremes of features 0..nf-1: the nf synthetic columns are gathered, the features split over ranks."""
    synth = comm.gather_rows(synth_local[:, :nf].contiguous())
    lo = (nf * comm.rank) // comm.world
    hi = (nf * (comm.rank + 1)) // comm.world
    dmax, dmin = np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
    if hi > lo:
        a, b = k.ks_extremes(real[:, lo:hi].contiguous(), synth[:, lo:hi].contiguous(), hi - lo)
        dmax[lo:hi], dmin[lo:hi] = a, b
    return comm.sum(dmax), comm.sum(dmin), int(synth.shape[0])


# ---- per-feature marginals over every column ---------------------------------------------------------------
MARGINAL_FIELDS = ("ks_dmax", "ks_dmin", "w1", "below", "above")
MARGINAL_GATHER_BYTES = 256 << 20      # the gathered synthetic columns of one chunk of sharded_marginals, at most


def sharded_marginals(comm: ShardComm, k, real, synth_local, chunk_cols: int = 0, gather_cols: int = 0) -> Dict[str, np.ndarray]:
    """The per-feature arrays of ``k.marginals`` (``MARGINAL_FIELDS``) over all D columns, plus ``n1`` and ``n2``, with the real cohort
    replicated and the synthetic rows sharded.  One column chunk at a time -- ``gather_cols`` columns, 0: as many as keep the gathered
    chunk within ``MARGINAL_GATHER_BYTES`` -- the chunk's synthetic columns are gathered (``gather_rows``), its features are split
    over the ranks, and every rank fills its own features' entries; the arrays are summed at the end (an entry is non-zero on one
    rank only, so the sum is that rank's value to the bit).  A rank holds one gathered chunk at a time, never [n2, D].  With an
    inactive ``comm`` this is one ``k.marginals`` call on the tensors as they are."""
    n1, D = int(real.shape[0]), int(real.shape[1])
    if int(synth_local.shape[1]) != D:
        raise ValueError("the cohorts must have the same features")
    n2 = int(comm.sum(int(synth_local.shape[0]))[0])
    if n1 < 1 or n2 < 1 or D < 1:
        raise ValueError("marginals need at least one row per cohort and one feature")
    if not comm.on:
        out = dict(k.marginals(real, synth_local, chunk_cols))
        out.update(n1=n1, n2=n2)
        return out
    width = int(gather_cols) if gather_cols else max(1, min(D, MARGINAL_GATHER_BYTES // (4 * n2)))
    out = {name: np.zeros(D, dtype=np.float64 if name == "w1" else np.int64) for name in MARGINAL_FIELDS}
    for c0 in range(0, D, width):
        c1 = min(D, c0 + width)
        synth = comm.gather_rows(synth_local[:, c0:c1].contiguous())
        lo = c0 + ((c1 - c0) * comm.rank) // comm.world
        hi = c0 + ((c1 - c0) * (comm.rank + 1)) // comm.world
        if hi > lo:
            part = k.marginals(real[:, lo:hi], synth[:, lo - c0:hi - c0], chunk_cols)
            for name in MARGINAL_FIELDS:
                out[name][lo:hi] = part[name]
    out = {name: comm.sum(v) for name, v in out.items()}
    out.update(n1=n1, n2=n2)
    return out


def real_center_and_sd(k, real):
    """``(center, sd)`` of every column of ``real``: the fp32-rounded mean (float32 [D]) and the sample standard deviation (ddof = 1,
    float64 [D]), from two ``k.col_centered_moments`` passes -- sums about 0 for the mean, then about the fp32-rounded mean, whose
    rounding the first moment takes out.  The sd is exactly 0 for a constant column (and for a one-row cohort)."""
    n = int(real.shape[0])
    s0, _ = k.col_centered_moments(real)
    center = (np.asarray(s0, dtype=np.float64) / n).astype(np.float32)
    s, q = k.col_centered_moments(real, center)
    if n < 2:
        return center, np.zeros(int(real.shape[1]), dtype=np.float64)
    var = (np.asarray(q, dtype=np.float64) - np.asarray(s, dtype=np.float64) ** 2 / n) / (n - 1)
    return center, np.sqrt(np.maximum(var, 0.0))


def real_sample_sd(k, real) -> np.ndarray:
    """float64 [D]: the sample standard deviation of ``real_center_and_sd``."""
    return real_center_and_sd(k, real)[1]


def marginal_ks(rows: Dict[str, np.ndarray]) -> np.ndarray:
    """float64 [D]: the two-sample KS distance max(dmax, -dmin) / (n1 n2) of every feature (scipy.stats.ks_2samp's statistic)."""
    dmax, dmin = np.asarray(rows["ks_dmax"], dtype=np.int64), np.asarray(rows["ks_dmin"], dtype=np.int64)
    return np.maximum(np.maximum(dmax, -dmin), 0).astype(np.float64) / (float(rows["n1"]) * float(rows["n2"]))


def marginal_summary(rows: Dict[str, np.ndarray], bounds: Sequence[int], names: Sequence[str]) -> Dict[str, float]:
    """The ``marginal_*`` figures from the per-feature arrays of ``sharded_marginals`` plus ``real_sd`` (``real_sample_sd``); pure host
    code.  Effect sizes only, no p-values: at 10^4-10^5 patients every feature is significant, and the Smirnov tail costs
    milliseconds per feature.

      ``marginal_features``, ``marginal_constant_features``  D, and the features whose real sd is 0: they keep their KS distance and
          range counts and are left out of the scaled W1 figures
      ``marginal_ks_mean / _median / _p95 / _max``, ``marginal_ks_max_feature``  over the KS distances; the last a column index
      ``marginal_w1_scaled_mean / _median / _p95 / _max``, ``marginal_w1_scaled_max_feature``  W1 in units of the real column's sample
          sd, over the non-constant features (NaN and -1 when there is none)
      ``marginal_out_of_range_share``  synthetic values outside their real column's [min, max], over all values;
      ``marginal_out_of_range_max``  the worst feature's share
      with more than one block, per block ``marginal_ks_mean_<block>``, ``marginal_ks_max_<block>``, ``marginal_w1_scaled_mean_<block>``

    ``bounds``: 0 = b_0 < ... < b_B = D, one name per block (``corr_block_bounds``).  Every value is a number."""
    nb = len(bounds) - 1
    if nb < 1 or len(names) != nb:
        raise ValueError("one name per column block")
    ks = marginal_ks(rows)
    D = ks.shape[0]
    if int(bounds[0]) != 0 or int(bounds[-1]) != D or any(int(a) >= int(b) for a, b in zip(bounds, bounds[1:])):
        raise ValueError(f"the block bounds must rise from 0 to {D}")
    w1, sd = np.asarray(rows["w1"], dtype=np.float64), np.asarray(rows["real_sd"], dtype=np.float64)
    outside = np.asarray(rows["below"], dtype=np.int64) + np.asarray(rows["above"], dtype=np.int64)
    if w1.shape != (D,) or sd.shape != (D,) or outside.shape != (D,):
        raise ValueError("one entry per feature in every array")
    n2 = int(rows["n2"])
    live = sd > 0
    scaled = np.full(D, np.nan)
    scaled[live] = w1[live] / sd[live]
    nan = float("nan")

    def over(v, fn):
        return float(fn(v)) if v.size else nan

    s = scaled[live]
    out = {
        "marginal_features": D,
        "marginal_constant_features": int(D - live.sum()),
        "marginal_ks_mean": float(ks.mean()),
        "marginal_ks_median": float(np.median(ks)),
        "marginal_ks_p95": float(np.quantile(ks, 0.95)),
        "marginal_ks_max": float(ks.max()),
        "marginal_ks_max_feature": int(np.argmax(ks)),
        "marginal_w1_scaled_mean": over(s, np.mean),
        "marginal_w1_scaled_median": over(s, np.median),
        "marginal_w1_scaled_p95": over(s, lambda v: np.quantile(v, 0.95)),
        "marginal_w1_scaled_max": over(s, np.max),
        "marginal_w1_scaled_max_feature": int(np.flatnonzero(live)[np.argmax(s)]) if s.size else -1,
        "marginal_out_of_range_share": float(int(outside.sum()) / (float(n2) * D)),
        "marginal_out_of_range_max": float(outside.max() / float(n2)),
    }
    if nb > 1:
        for name, lo, hi in zip(names, bounds, bounds[1:]):
            out[f"marginal_ks_mean_{name}"] = float(ks[lo:hi].mean())
            out[f"marginal_ks_max_{name}"] = float(ks[lo:hi].max())
            out[f"marginal_w1_scaled_mean_{name}"] = over(scaled[lo:hi][live[lo:hi]], np.mean)
    return out


def sharded_mean_offdiag(comm: ShardComm, k, data_local, cols: Sequence[int]) -> float:
    """Mean off-diagonal Pearson correlation of data[:, cols] (utils/validation.py:156-161) over row shards."""
    g = len(cols)
    if g < 2:
        raise ValueError("a mean off-diagonal correlation needs at least 2 columns")
    s, q = k.col_moments(data_local, cols)
    tot = comm.sum(np.concatenate([s, q, [float(data_local.shape[0])]]))
    rows = tot[-1]
    mu = tot[:g] / rows
    var = (tot[g:2 * g] - rows * mu * mu) / (rows - 1)              # ddof = 1, as pandas .corr()
    with np.errstate(divide="ignore", invalid="ignore"):
        isd = np.where(var > 0, 1.0 / np.sqrt(var), np.nan)        # constant column -> NaN, as pandas
    S = float(comm.sum(k.rowz_sq(data_local, cols, mu, isd))[0])
    return (S / (rows - 1) - g) / (float(g) * (g - 1))


def sharded_pearson(comm: ShardComm, k, a_local, col_a: int, b_local, col_b: int) -> float:
    h = comm.sum(np.concatenate([k.pearson_sums(a_local, col_a, b_local, col_b), [float(a_local.shape[0])]]))
    n = h[5]
    cov, va, vb = h[4] - h[0] * h[1] / n, h[2] - h[0] * h[0] / n, h[3] - h[1] * h[1] / n
    return float(cov / np.sqrt(va * vb))


def sharded_nearest_records(comm: ShardComm, k, train, synth_local, holdout=None) -> Dict[str, np.ndarray]:
    """Per-row nearest-record distances of the privacy audit: the synthetic rows are this rank's shard, the real cohorts are
    replicated.  Every rank returns the arrays of the concatenated rows (float64 distances, int64 indices):
    ``dcr`` / ``match`` distance to and index of the nearest train row, ``second`` distance to the second nearest (a second pass
    that excludes the first match), ``real_nn`` each train row's distance to its nearest OTHER train row (the train rows are
    split over the ranks as queries), ``dcr_holdout`` distance to the nearest holdout row (only with a holdout)."""
    from .parallel import shard_rows

    def nearest(q, r, exclude=None):
        if q.shape[0] == 0:                              # an empty shard asks nothing of the kernel
            return torch.empty(0, dtype=torch.float32, device=q.device), torch.empty(0, dtype=torch.int32, device=q.device)
        return k.nearest(q, r, exclude)

    def dist(d2):
        return np.sqrt(comm.gather_rows(d2).detach().cpu().numpy().astype(np.float64))

    d2, match = nearest(synth_local, train)
    d2_second, _ = nearest(synth_local, train, match)
    lo, cnt = shard_rows(train.shape[0], comm.rank, comm.world)
    own = torch.arange(lo, lo + cnt, dtype=torch.int32, device=train.device)
    d2_real, _ = nearest(train[lo:lo + cnt].contiguous(), train, own)
    rows = {"dcr": dist(d2), "match": comm.gather_rows(match).detach().cpu().numpy().astype(np.int64), "second": dist(d2_second),
            "real_nn": dist(d2_real)}
    if holdout is not None:
        rows["dcr_holdout"] = dist(nearest(synth_local, holdout)[0])
    return rows


def privacy_summary(rows: Dict[str, np.ndarray]) -> Dict[str, float]:
    """The privacy figures from the per-row arrays of ``sharded_nearest_records`` (float64, numpy.quantile's default)."""
    dcr = np.asarray(rows["dcr"], dtype=np.float64)
    second = np.asarray(rows["second"], dtype=np.float64)
    real_nn = np.asarray(rows["real_nn"], dtype=np.float64)
    match = np.asarray(rows["match"], dtype=np.int64)
    if dcr.size == 0:
        raise ValueError("a privacy summary needs at least one synthetic row")
    with np.errstate(divide="ignore", invalid="ignore"):
        nndr = dcr / second                              # an infinite second neighbour (a one-row cohort) gives 0.0
    nndr[np.isnan(nndr)] = 0.0                           # 0/0: a row that copies two identical records
    out = {
        "privacy_dcr_min": float(dcr.min()),
        "privacy_dcr_p05": float(np.quantile(dcr, 0.05)),
        "privacy_dcr_median": float(np.median(dcr)),
        "privacy_exact_copy_fraction": float(np.mean(dcr == 0)),
        "privacy_nndr_p05": float(np.quantile(nndr, 0.05)),
        "privacy_nndr_median": float(np.median(nndr)),
        "privacy_real_nn_median": float(np.median(real_nn)),
        "privacy_closer_than_real_nn_fraction": float(np.mean(dcr < real_nn[match])),
    }
    if "dcr_holdout" in rows:
        dh = np.asarray(rows["dcr_holdout"], dtype=np.float64)
        out["privacy_holdout_dcr_median"] = float(np.median(dh))
        out["privacy_closer_to_train_fraction"] = float(np.mean((dcr < dh) + 0.5 * (dcr == dh)))
    return out


def prdc_summary(rows: Dict[str, np.ndarray], k: int) -> Dict[str, float]:
    """Precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) from the per-row counts of
    ``BiologicalValidator.fidelity_diversity`` (int64 counts, float64 means).  With X the N real rows, Y the M synthetic rows and
    r_k(.) a row's distance to its k-th nearest neighbour inside its own cohort, itself excluded, the four figures are means over

      ``synth_in_real_balls`` [M]  #{i : d(y_j, x_i) <= r_k(x_i)}      precision = mean(count > 0);  density = sum / (k M)
      ``real_in_synth_balls`` [N]  #{j : d(x_i, y_j) <= r_k(y_j)}      recall    = mean(count > 0)
      ``real_ball_synth``     [N]  #{j : d(x_i, y_j) <= r_k(x_i)}      coverage  = mean(count > 0)

    (precision and density read the same array).  Other keys of ``rows`` -- the radii -- are ignored."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    a = np.asarray(rows["synth_in_real_balls"], dtype=np.int64)
    b = np.asarray(rows["real_in_synth_balls"], dtype=np.int64)
    c = np.asarray(rows["real_ball_synth"], dtype=np.int64)
    if a.size == 0 or b.size == 0:
        raise ValueError("a precision / recall summary needs at least one row in each cohort")
    if b.shape != c.shape:
        raise ValueError("real_in_synth_balls and real_ball_synth must have one entry per real row")
    return {
        "prdc_precision": float(np.mean(a > 0)),
        "prdc_recall": float(np.mean(b > 0)),
        "prdc_density": float(a.sum(dtype=np.int64) / (float(k) * a.size)),
        "prdc_coverage": float(np.mean(c > 0)),
        "prdc_k": k,
    }


def sharded_centered_gram(comm: ShardComm, k, local_rows):
    """(n, mu, G): row count, float64 column means (numpy) and the float64 [D, D] centred cross-product sum_r (x_r - mu)(x_r - mu)^T of
    the concatenated row shards, on ``local_rows``' device.  Column sums and row counts are all-reduced to the double mean mu, every
    rank runs ``k.centered_gram`` with the centre c = float32(mu) -- the kernel subtracts in fp32 --, G is all-reduced, and the
    rounding of the centre is taken out in double: sum (x - c)(x - c)^T = sum (x - mu)(x - mu)^T + n (mu - c)(mu - c)^T exactly.
    An empty shard contributes nothing.  With an inactive ``comm`` this is the unsharded path."""
    rows, D = int(local_rows.shape[0]), int(local_rows.shape[1])
    sums = k.column_sums(local_rows) if rows else np.zeros(D, dtype=np.float64)
    tot = comm.sum(np.concatenate([np.asarray(sums, dtype=np.float64), [float(rows)]]))
    n = int(round(tot[-1]))
    if n < 1:
        raise ValueError("a centred Gram matrix needs at least one row")
    mu = tot[:D] / n
    c = mu.astype(np.float32)
    if rows:
        g = k.centered_gram(local_rows, c)
    else:
        g = torch.zeros((D, D), dtype=torch.float64, device=local_rows.device)
    g = comm.sum_tensor(g)
    d = torch.from_numpy(mu - c.astype(np.float64)).to(g.device)
    g.sub_(torch.outer(d, d).mul_(float(n)))
    return n, mu, g


def frechet_distance(mu1, S1, mu2, S2) -> Dict[str, float]:
    """Squared Frechet (2-Wasserstein) distance between the Gaussians N(mu1, S1) and N(mu2, S2), as FID reports it:
    |mu1 - mu2|^2 + tr(S1 + S2 - 2 (S1 S2)^(1/2)).  numpy float64 throughout and symmetric eigen-decompositions only: with
    A = S1^(1/2) from eigh(S1) (negative eigenvalues clipped to 0), tr (S1 S2)^(1/2) = sum sqrt(eigvalsh(A S2 A)) (clipped), so
    rank-deficient covariances -- fewer patients than features -- give a finite, non-negative value where a general matrix
    square root does not.  Keys: ``frechet_distance``, ``frechet_mean_term``, ``frechet_cov_term``."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    S1, S2 = np.atleast_2d(np.asarray(S1, dtype=np.float64)), np.atleast_2d(np.asarray(S2, dtype=np.float64))
    D = mu1.shape[0]
    if mu1.shape != (D,) or mu2.shape != (D,) or S1.shape != (D, D) or S2.shape != (D, D):
        raise ValueError("frechet_distance needs two means [D] and two covariances [D, D]")
    if not (np.isfinite(mu1).all() and np.isfinite(mu2).all() and np.isfinite(S1).all() and np.isfinite(S2).all()):
        raise ValueError("frechet_distance needs finite moments")
    S1, S2 = 0.5 * (S1 + S1.T), 0.5 * (S2 + S2.T)
    def clipped(lam):
        # negative eigenvalues, and those inside the rounding noise of the largest (numpy.linalg.matrix_rank's tolerance), are zero:
        # the square root would turn a null eigenvalue's 1e-16 of noise into 1e-8
        top = float(lam.max(initial=0.0))
        return np.where(lam > D * np.finfo(np.float64).eps * top, lam, 0.0)

    w, v = np.linalg.eigh(S1)
    a = (v * np.sqrt(clipped(w))) @ v.T
    m = a @ S2 @ a
    lam = clipped(np.linalg.eigvalsh(0.5 * (m + m.T)))
    diff = mu1 - mu2
    mean_term = float(diff @ diff)
    cov_term = max(float(np.trace(S1) + np.trace(S2) - 2.0 * np.sqrt(lam).sum()), 0.0)
    return {"frechet_distance": max(mean_term + cov_term, 0.0), "frechet_mean_term": mean_term, "frechet_cov_term": cov_term}


def corr_block_bounds(blocks, D: int):
    """(bounds, names) of a ``{name: width}`` mapping in column order (None: one block, "all"); the widths must add up to D."""
    if blocks is None:
        return [0, int(D)], ["all"]
    names, bounds = [], [0]
    for name, width in blocks.items():
        width = int(width)
        if width < 0:
            raise ValueError(f"block {name!r} has a negative width")
        if width == 0:
            continue
        names.append(str(name))
        bounds.append(bounds[-1] + width)
    if bounds[-1] != int(D):
        raise ValueError(f"the block widths add up to {bounds[-1]}, the cohorts have {D} features")
    return bounds, names


def corr_summary(stats: Dict[str, np.ndarray], bounds: Sequence[int], names: Sequence[str]) -> Dict[str, float]:
    """The ``corr_*`` figures from the per-block-pair sums of ``DeviceKernels.corr_compare`` (pairs i < j of non-constant columns,
    delta = r_synth - r_real): mean, root mean square and largest |delta|, the Frobenius norm of the difference of the two correlation
    matrices (sqrt(2 sum delta^2): both triangles, the diagonals agree), the pair and constant-column counts, and over the STRONG pairs
    (|r_real| >= the threshold ``corr_compare`` was given) their number, the share whose r_synth has r_real's sign and their mean
    |delta| -- NaN where there is no strong pair (or no pair at all).  With more than one block also ``corr_mean_abs_diff_<a>_<b>``
    for every block pair a <= b in row-major order."""
    nb = len(bounds) - 1
    if nb < 1 or len(names) != nb:
        raise ValueError("one name per column block")
    n_pairs = nb * (nb + 1) // 2
    pairs = np.asarray(stats["pairs"], dtype=np.int64)
    if pairs.shape != (n_pairs,):
        raise ValueError(f"{nb} blocks make {n_pairs} block pairs, the sums hold {pairs.shape}")
    sum_abs, sum_sq = np.asarray(stats["sum_abs"], dtype=np.float64), np.asarray(stats["sum_sq"], dtype=np.float64)
    total = int(pairs.sum())
    strong = int(np.asarray(stats["strong_pairs"], dtype=np.int64).sum())
    agree = int(np.asarray(stats["strong_agree"], dtype=np.int64).sum())
    nan = float("nan")
    out = {
        "corr_mean_abs_diff": float(sum_abs.sum() / total) if total else nan,
        "corr_rms_diff": float(np.sqrt(sum_sq.sum() / total)) if total else nan,
        "corr_max_abs_diff": float(np.max(np.asarray(stats["max_abs"], dtype=np.float64))) if total else nan,
        "corr_frobenius_diff": float(np.sqrt(2.0 * sum_sq.sum())),
        "corr_pairs": total,
        "corr_constant_columns": int(stats["constant_columns"]),
        "corr_strong_pairs": strong,
        "corr_strong_sign_agreement": float(agree / strong) if strong else nan,
        "corr_strong_mean_abs_diff": float(np.asarray(stats["strong_sum_abs"], dtype=np.float64).sum() / strong) if strong else nan,
    }
    if nb > 1:
        p = 0
        for a in range(nb):
            for b in range(a, nb):
                out[f"corr_mean_abs_diff_{names[a]}_{names[b]}"] = float(sum_abs[p] / pairs[p]) if pairs[p] else nan
                p += 1
    return out


# ---- downstream utility: fits of regularised linear heads over row shards -------------------------------
GLM_RUN_ROWS = L.OSD_GLM_RUN_ROWS       # rows one fp32 gradient run of osd_val_glm_eval (and of osd_val_cox_eval) covers
CONC_I_TILE, CONC_J_CHUNK = L.OSD_CONC_I_TILE, L.OSD_CONC_J_CHUNK      # rows of a workgroup and partners of an LDS chunk of osd_val_concordance
COXS_ROWS = L.OSD_COXS_ROWS             # positions of one work item of osd_val_cox_score


def pooled_standardisation(k, parts):
    """(n, center, scale) of the rows of ``parts`` -- a list of (comm, rows): ShardComm(False) for a replicated tensor, the
    validator's for a row shard -- taken together: n the row count, center the float32 column means the kernel subtracts, scale
    float32 1 / sd (population sd about the float64 mean; 0 for a constant column, which drops it).  Two passes: column sums, then
    ``k.col_centered_moments`` about the fp32 centre, each all-reduced and added over the parts."""
    D = int(parts[0][1].shape[1])
    tot = np.zeros(D + 1, dtype=np.float64)
    for comm, t in parts:
        rows = int(t.shape[0])
        sums = k.column_sums(t) if rows else np.zeros(D, dtype=np.float64)
        tot += comm.sum(np.concatenate([np.asarray(sums, dtype=np.float64), [float(rows)]]))
    n = int(round(tot[-1]))
    if n < 2:
        raise ValueError("a standardisation needs at least 2 rows")
    center = (tot[:D] / n).astype(np.float32)
    mom = np.zeros(2 * D, dtype=np.float64)
    for comm, t in parts:
        if int(t.shape[0]):
            s, q = k.col_centered_moments(t, center)
            mom += comm.sum(np.concatenate([s, q]))
        else:
            mom += comm.sum(np.zeros(2 * D, dtype=np.float64))
    shift = mom[:D] / n
    var = mom[D:] / n - shift * shift
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(var > 0, 1.0 / np.sqrt(np.where(var > 0, var, 1.0)), 0.0)
    return n, center, scale.astype(np.float32)


def glm_sums(k, parts, center, scale, W, kinds):
    """(loss [K], grad [K, D + 1]) float64: the sums of ``k.glm_eval`` over ``parts`` -- a list of (comm, rows, targets, row weights
    or None) --, each part's all-reduced over its communicator and the parts added in double; an empty shard contributes zeros.  This
    is the ``eval_fn`` of ``utility.fit_glm``."""
    K, D = len(kinds), int(parts[0][1].shape[1])
    tot = np.zeros(K * (D + 2), dtype=np.float64)
    for comm, x, y, a in parts:
        if int(x.shape[0]):
            loss, grad, _ = k.glm_eval(x, center, scale, y, W, kinds, row_weight=a)
            flat = np.concatenate([np.asarray(loss, dtype=np.float64), np.asarray(grad, dtype=np.float64).ravel()])
        else:
            flat = np.zeros(K * (D + 2), dtype=np.float64)
        tot += comm.sum(flat)
    return tot[:K], tot[K:].reshape(K, D + 1)


def fit_heads(k, parts, center, scale, kinds, n: float, l2: float, max_iter: int = 200, tol: float = 1e-5):
    """W float64 [K, D + 1] of ``utility.fit_glm`` over ``parts`` (as ``glm_sums`` takes them), the heads in groups of at most four
    -- one kernel call per group and iteration --, and the list of the groups' fit reports."""
    K, D = len(kinds), int(parts[0][1].shape[1])
    W = np.zeros((K, D + 1), dtype=np.float64)
    reports = []
    for lo in range(0, K, U.MAX_HEADS):
        hi = min(K, lo + U.MAX_HEADS)
        sub = [(comm, x, y[:, lo:hi].contiguous(), a) for comm, x, y, a in parts]
        fit = U.fit_glm(lambda w: glm_sums(k, sub, center, scale, w, kinds[lo:hi]), hi - lo, D, kinds[lo:hi], n, l2, max_iter=max_iter,
                        tol=tol)
        W[lo:hi] = fit["W"]
        reports.append(fit)
    return W, reports


def glm_scores(k, x, center, scale, W, kinds) -> np.ndarray:
    """float64 [rows, K] numpy: the scores z of the rows of x under W, the heads in groups of at most four."""
    K = len(kinds)
    out = np.zeros((int(x.shape[0]), K), dtype=np.float64)
    if int(x.shape[0]) == 0:
        return out
    for lo in range(0, K, U.MAX_HEADS):
        hi = min(K, lo + U.MAX_HEADS)
        _, _, z = k.glm_eval(x, center, scale, None, W[lo:hi], kinds[lo:hi], grad=False, scores=True)
        out[:, lo:hi] = z.detach().cpu().numpy().astype(np.float64)
    return out


def utility_metrics(comm: ShardComm, k, x_train, c_train, x_synth, c_synth, x_test, c_test, names, l2: float = 1e-2,
                    max_iter: int = 200, tol: float = 1e-5) -> Dict[str, float]:
    """``BiologicalValidator.downstream_utility`` on tensors: the feature matrices on the kernels' device, the condition matrices
    float64 numpy [rows, K]; ``x_synth`` / ``c_synth`` are this rank's row shard when ``comm`` is active.  ``k`` needs
    ``column_sums``, ``col_centered_moments`` and ``glm_eval`` (DeviceKernels, or a float64 stand-in in the tests)."""
    one = ShardComm(False)
    c_train, c_synth, c_test = (np.asarray(c, dtype=np.float64) for c in (c_train, c_synth, c_test))
    K = c_train.shape[1]
    off_binary = comm.sum(np.array([float((~np.isin(c_synth[:, j], (0.0, 1.0))).sum()) for j in range(K)]))
    kinds = [U.LOGISTIC if off_binary[j] == 0 and h == U.LOGISTIC else U.SQUARED for j, h in enumerate(U.head_kinds([c_train, c_test]))]
    scores, targets = [], []
    for label, cm, x, c in (("synthetic", comm, x_synth, c_synth), ("real_train", one, x_train, c_train)):
        tot = cm.sum(np.concatenate([c.sum(0), [float(c.shape[0])]]))
        n, mean = tot[-1], tot[:K] / tot[-1]
        sd = np.sqrt(cm.sum(((c - mean) ** 2).sum(0)) / n)
        mu, inv = np.zeros(K), np.ones(K)
        for j, name in enumerate(names):
            if kinds[j] == U.LOGISTIC:
                for where, share in ((label, mean[j]), ("real_test", c_test[:, j].mean())):
                    if share <= 0.0 or share >= 1.0:
                        raise ValueError(f"condition {name!r} has a single class in the {where} cohort: no AUC can be computed")
            elif not sd[j] > 0:
                raise ValueError(f"condition {name!r} is constant in the {label} cohort: it cannot be standardised")
            else:
                mu[j], inv[j] = mean[j], 1.0 / sd[j]
        y = torch.from_numpy(((c - mu) * inv).astype(np.float32)).to(x.device)
        n_rows, center, scale = pooled_standardisation(k, [(cm, x)])
        W, _ = fit_heads(k, [(cm, x, y, None)], center, scale, kinds, float(n_rows), l2, max_iter=max_iter, tol=tol)
        scores.append(glm_scores(k, x_test, center, scale, W, kinds))
        targets.append((c_test - mu) * inv)
    return U.utility_summary(names, kinds, scores[0], scores[1], targets[0], targets[1])


def c2st_metrics(comm: ShardComm, k, x_real, x_synth, test_fraction: float = 0.3, seed: int = 0, l2: float = 1e-2, max_iter: int = 200,
                 tol: float = 1e-5) -> Dict[str, float]:
    """``BiologicalValidator.discriminator_test`` on device tensors; ``x_synth`` is this rank's row shard when ``comm`` is active.
    The synthetic split is a seeded permutation of the GLOBAL row numbers (rank order), so it does not depend on the sharding."""
    from .parallel import _one_hot
    one = ShardComm(False)
    n_r, local = int(x_real.shape[0]), int(x_synth.shape[0])
    counts = comm.sum(_one_hot(comm.rank, comm.world) * local).astype(np.int64)
    n_s, off = int(counts.sum()), int(counts[:comm.rank].sum())
    tr_r, te_r = U.split_indices(n_r, test_fraction, seed)
    tr_s, te_s = U.split_indices(n_s, test_fraction, seed + 1)

    def take(t, idx, lo=0, cnt=None):
        idx = idx[(idx >= lo) & (idx < lo + (t.shape[0] if cnt is None else cnt))] - lo
        return t.index_select(0, torch.as_tensor(idx, dtype=torch.int64, device=t.device))

    xr_tr, xr_te = take(x_real, tr_r), take(x_real, te_r)
    xs_tr, xs_te = take(x_synth, tr_s, off, local), take(x_synth, te_s, off, local)
    n, center, scale = pooled_standardisation(k, [(one, xr_tr), (comm, xs_tr)])
    # row weights that give the two classes the same total weight, n / 2 each
    w_r, w_s = n / (2.0 * len(tr_r)), n / (2.0 * len(tr_s))
    dev = x_real.device
    parts = [(one, xr_tr, torch.zeros((xr_tr.shape[0], 1), device=dev), torch.full((xr_tr.shape[0],), w_r, device=dev)),
             (comm, xs_tr, torch.ones((xs_tr.shape[0], 1), device=dev), torch.full((xs_tr.shape[0],), w_s, device=dev))]
    kinds = [U.LOGISTIC]
    W, _ = fit_heads(k, parts, center, scale, kinds, float(n), l2, max_iter=max_iter, tol=tol)
    z_r = glm_scores(k, xr_te, center, scale, W, kinds)
    z_s = comm.gather_rows(torch.from_numpy(glm_scores(k, xs_te, center, scale, W, kinds))).numpy()
    return U.c2st_summary(z_r, z_s)


# ---- survival utility: Cox fits and concordance ----------------------------------------------------------
def survival_metrics(k, x_train, s_train, x_synth, s_synth, x_test, s_test, l2: float = 1e-2, max_iter: int = 200, tol: float = 1e-5,
                     return_fits: bool = False):
    """``BiologicalValidator.survival_utility`` on tensors: the feature matrices on the kernels' device, the survival matrices float64
    numpy [rows, 2] = (time, event).  ``k`` needs ``column_sums``, ``col_centered_moments``, ``glm_eval``, ``cox_plan``, ``cox_eval``
    and ``concordance`` (DeviceKernels, or a float64 stand-in in the tests).  ``return_fits=True`` also returns the two fit reports
    of ``survival.fit_cox``, each with its ``center`` and ``scale``, synthetic first."""
    one = ShardComm(False)
    surv = {"real_train": np.asarray(s_train, dtype=np.float64), "synthetic": np.asarray(s_synth, dtype=np.float64),
            "real_test": np.asarray(s_test, dtype=np.float64)}
    shares = {}
    for label, s in surv.items():
        if not np.isin(s[:, 1], (0.0, 1.0)).all():
            raise ValueError(f"the event flags of {label} must be 0 or 1")
        shares[label] = float(s[:, 1].mean())
        if not shares[label] > 0.0:
            raise ValueError(f"the {label} cohort has no event: a Cox model cannot be fitted or scored on it")
    D = int(x_test.shape[1])
    coefs, counts, fits = [], [], []
    for label, x in (("synthetic", x_synth), ("real_train", x_train)):
        n_rows, center, scale = pooled_standardisation(k, [(one, x)])
        with k.cox_plan(surv[label][:, 0], surv[label][:, 1]) as plan:
            fit = SV.fit_cox(lambda w: k.cox_eval(x, center, scale, w, plan)[:2], D, float(n_rows), l2, max_iter=max_iter, tol=tol)
        W = np.concatenate([fit["w"], [0.0]])[None, :]
        risk = glm_scores(k, x_test, center, scale, W, [U.SQUARED])[:, 0]
        c = k.concordance(surv["real_test"][:, 0], surv["real_test"][:, 1], risk)
        if c[0] <= 0:
            raise ValueError("the real_test cohort has no comparable pair: no event is followed by a later time")
        coefs.append(fit["w"] * scale.astype(np.float64))
        counts.append(c)
        fits.append(dict(fit, center=center, scale=scale))
    out = SV.survival_summary(coefs[0], coefs[1], counts[0], counts[1], shares)
    return (out, fits) if return_fits else out


# ---- prognostic-gene fidelity: one Cox model per feature and cohort -----------------------------------------
def prognostic_metrics(k, x, s_real, y, s_synth, bounds=None, block_names=None, alpha: float = 0.05, top_k: int = 50,
                       mle: bool = True):
    """``BiologicalValidator.prognostic_fidelity`` on tensors: ``(summary, rows)``, the feature matrices on the kernels' device, the
    survival matrices float64 numpy [rows, 2] = (time, event).  ``k`` needs ``col_centered_moments``, ``cox_plan`` and ``cox_score``
    (DeviceKernels, or a float64 stand-in in the tests).  ``rows`` holds both screens over ALL features (``survival.cox_screen``;
    a constant real column has scale 0 and NaNs), ``center``, ``scale`` and ``live``, the mask of the features the summary is over."""
    surv = {"real": np.asarray(s_real, dtype=np.float64), "synthetic": np.asarray(s_synth, dtype=np.float64)}
    D = int(x.shape[1])
    for label, t in (("real", x), ("synthetic", y)):
        s = surv[label]
        if s.ndim != 2 or s.shape != (int(t.shape[0]), 2):
            raise ValueError(f"the survival matrix of {label} must be [{int(t.shape[0])}, 2] = (time, event), got {s.shape}")
        if not np.isfinite(s[:, 0]).all() or not np.isin(s[:, 1], (0.0, 1.0)).all():
            raise ValueError(f"the times of {label} must be finite and its event flags 0 or 1")
        if not s[:, 1].any():
            raise ValueError(f"the {label} cohort has no event: no feature can be prognostic in it")
    center, sd = real_center_and_sd(k, x)
    live = sd > 0
    with np.errstate(divide="ignore"):
        scale = np.where(live, 1.0 / np.where(live, sd, 1.0), 0.0).astype(np.float32)
    live &= scale > 0                                            # (a spread so large that 1 / sd is no fp32 number drops the column too)
    if not live.any():
        raise ValueError("every column of the real cohort is constant")
    screens = {}
    for label, t in (("real", x), ("synthetic", y)):
        with k.cox_plan(surv[label][:, 0], surv[label][:, 1]) as plan:
            screens[label] = SV.cox_screen(k, t, plan, center, scale, mle=mle)
    idx = np.nonzero(live)[0]
    sides = []
    for label in ("real", "synthetic"):
        e, q = screens[label]["effect"][idx], screens[label]["q"][idx]
        dead = ~(np.isfinite(e) & np.isfinite(q))                # no information in this cohort (a constant synthetic column): no signal
        sides.append({"effect": np.where(dead, 0.0, e), "q": np.where(dead, 1.0, q)})
    if bounds is not None and len(bounds) > 2:                   # the blocks' bounds among the live features
        bounds = [int((idx < b).sum()) for b in bounds]
    one = DE.contrast_summary(sides[0], sides[1], alpha, top_k, bounds, block_names)
    one["max_gap_feature"] = int(idx[one["max_gap_feature"]])
    summary = {f"prog_{key}": v for key, v in one.items()}
    summary["prog_features"] = int(live.sum())
    summary["prog_constant_features"] = int(D - live.sum())
    for label, short in (("real", "real"), ("synthetic", "synth")):
        scr = screens[label]
        summary[f"prog_not_converged_{short}"] = int((~scr["converged"][idx]).sum())
        summary[f"prog_events_{short}"] = int(surv[label][:, 1].sum())
        z = np.abs(scr["z_score"][idx])
        summary[f"prog_max_abs_z_{short}"] = float(np.nanmax(z)) if np.isfinite(z).any() else float("nan")
    rows = {"real": screens["real"], "synthetic": screens["synthetic"], "center": center, "scale": scale, "live": live}
    return summary, rows


class BiologicalValidator:
    """utils/validation.py:18 -- device versions of the metrics named in the module docstring."""

    def __init__(self, config: dict, device: str = "cuda", sharded: bool = False):
        self.config = config
        ev = config.get("evaluation", {})
        self.driver_genes = ev.get("driver_genes", [])
        self.mutually_exclusive_pairs = ev.get("mutually_exclusive_pairs", [])
        self.required_correlations = ev.get("required_correlations", [])
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the validation kernels run on a ROCm device; there is no CPU fallback")
        self.k = DeviceKernels(self.device)
        self.sharded = bool(sharded)
        self.comm = ShardComm(sharded)            # synthetic rows sharded over ranks when active
        self._one = ShardComm(False)              # the replicated real cohort never communicates

    def _agree(self, result):
        """Sharded mode: every rank reports rank 0's value (partial sums replicated per rank, e.g. over the real cohort,
        can differ in the last bit between ranks because double atomics commit in any order)."""
        return self.comm.bcast_object(result)

    # -- utils/validation.py:273-298 ----------------------------------------------------------
    def compute_mmd(self, X, Y, kernel: str = "rbf", gamma: Optional[float] = None) -> float:
        if kernel != "rbf":
            raise ValueError("only the rbf kernel exists in the reference")
        x, y = _dev(X, self.device), _dev(Y, self.device)
        if x.shape[1] != y.shape[1]:
            raise ValueError("X and Y must have the same number of features")
        if not self.comm.on:
            out = C.c_double()
            L.check(L.lib().osd_val_mmd(self.k._stream(), self.k.index, L.ptr(x), x.shape[0], L.ptr(y), y.shape[0], x.shape[1],
                                        float(gamma) if gamma else 0.0, C.byref(out)))
            return float(out.value)
        return self._agree(sharded_mmd(self.comm, self.k, x, y, float(gamma) if gamma else 1.0 / x.shape[1]))

    def ks_tests(self, real_data, synthetic_data, max_features: int = 100):
        """Per-feature (statistic, p-value) arrays for the first min(D, 100) features."""
        r, s = _dev(real_data, self.device), _dev(synthetic_data, self.device)
        nf = min(r.shape[1], max_features)
        dmax, dmin, n2 = sharded_ks_extremes(self.comm, self.k, r, s, nf)
        return self._agree(_ks_pvalues(r.shape[0], n2, dmax[:nf], dmin[:nf]))

    # -- utils/validation.py:225-271 --------------------------------------------------------------
    def statistical_tests(self, real_data, synthetic_data, pca: str = "host") -> Dict[str, float]:
        """The reference's figures: KS p-values over the first min(D, 100) columns, the MMD and the Wasserstein distance on 10
        principal components.  The check of EVERY feature's marginal lives in ``marginal_fidelity``.
        ``pca="host"`` (the default) is the reference's own route to ``wasserstein_distance_mean``: both cohorts are downloaded and
        sklearn's ``PCA(10)`` runs on a side thread.  ``pca="device"`` takes the figure from a ``pca.DevicePCA(10)`` fit on the real
        cohort (block subspace iteration), fp32 scores of both cohorts and one ``DeviceKernels.marginals``
        call: no cohort is downloaded for it, and the draws from numpy's GLOBAL generator that sklearn's randomized solver makes on
        the host path are then NOT made (the device fit has its own ``RandomState(0)``), so code that relies on the state of that
        generator after this call sees another state.  The two routes agree to the rounding of the fp32 scores where sklearn's
        solver is exact, and to its own approximation error where it is randomized."""
        if pca not in ("host", "device"):
            raise ValueError('pca must be "host" or "device"')
        logger.info("Running statistical tests...")
        # The device parts first -- KS extremes (exact integers), then the MMD Gram blocks -- with the reference's own host-side parts
        # BESIDE the MMD on two threads (the ctypes call releases the GIL): the 100 Smirnov p-values (scipy's kstwo.sf: 8 ms each at
        # N = 62 500, whether called once or a hundred times) and the PCA fit + projection behind the Wasserstein figure (:256-269;
        # the reference's own sklearn / scipy calls; fitted on the replicated real data, each rank projects its shard, the 10
        # projected columns are gathered).  Same calls, same inputs, same order of draws from numpy's global generator (only the PCA
        # draws): only the wall time moves -- 4.7 s -> 2.4 s per 125 000-row scenario together with the triangular MMD.
        import threading
        from scipy import stats
        from sklearn.decomposition import PCA
        r, s = _dev(real_data, self.device), _dev(synthetic_data, self.device)
        nf = min(r.shape[1], 100)
        dmax, dmin, n2 = sharded_ks_extremes(self.comm, self.k, r, s, nf)
        if pca == "host":
            real_host, synth_host = _host(real_data), _host(synthetic_data)      # device -> host before the MMD kernels occupy the stream
        box = {}

        def guarded(key, fn):
            def run():
                try:
                    box[key] = fn()
                except BaseException as e:               # re-raised on the calling thread
                    box["error"] = e
            return threading.Thread(target=run)

        def fit():
            pca = PCA(n_components=10)
            return pca.fit_transform(real_host), pca.transform(synth_host)

        threads = [guarded("ks", lambda: _ks_pvalues(r.shape[0], n2, dmax[:nf], dmin[:nf]))] + ([guarded("pca", fit)] if pca == "host" else [])
        for th in threads:
            th.start()
        results = {}
        try:
            results["mmd"] = self.compute_mmd(real_data, synthetic_data)
        finally:
            for th in threads:
                th.join()
        if "error" in box:
            raise box["error"]
        _, pvals = self._agree(box["ks"])
        results = {"ks_test_mean_pvalue": float(np.mean(pvals)), "ks_test_fraction_significant": float((pvals < 0.05).mean()), "mmd": results["mmd"]}
        logger.info(f"KS test mean p-value: {results['ks_test_mean_pvalue']:.3f}")
        logger.info(f"KS test fraction significant: {results['ks_test_fraction_significant']:.3f}")
        logger.info(f"MMD: {results['mmd']:.4f}")
        if pca == "device":
            fitted = PC.DevicePCA(10).fit(r, kernels=self.k)
            real_scores = fitted.transform(r, kernels=self.k)
            synth_scores = self.comm.gather_rows(fitted.transform(s, kernels=self.k).contiguous())
            results["wasserstein_distance_mean"] = float(np.mean(self.k.marginals(real_scores, synth_scores)["w1"]))
        else:
            real_pca, synth_pca = box["pca"]
            if self.comm.on:
                synth_pca = self.comm.gather_rows(torch.from_numpy(np.ascontiguousarray(synth_pca))).numpy()
            results["wasserstein_distance_mean"] = float(np.mean([stats.wasserstein_distance(real_pca[:, i], synth_pca[:, i]) for i in range(10)]))
        logger.info(f"Mean Wasserstein distance: {results['wasserstein_distance_mean']:.3f}")
        return self._agree(results)

    # -- privacy: distances to the nearest real record (no counterpart in the reference) ---------
    def privacy_audit(self, real_train, synthetic, real_holdout=None, return_rows: bool = False):
        """Distance-to-closest-record figures of ``synthetic`` (this rank's shard when sharded) against the cohort the model was
        trained on, and against a holdout cohort when one is given: the ``privacy_*`` keys of ``privacy_summary``.  Distances
        are plain Euclidean over the columns as given -- callers scale their inputs.  ``return_rows=True`` also returns the
        per-row arrays of ``sharded_nearest_records``."""
        tr, sy = _dev(real_train, self.device), _dev(synthetic, self.device)
        ho = None if real_holdout is None else _dev(real_holdout, self.device)
        for name, t in (("real_train", tr), ("synthetic", sy), ("real_holdout", ho)):
            if t is None:
                continue
            if t.dim() != 2 or t.shape[1] != tr.shape[1]:
                raise ValueError(f"{name} must be [rows, {tr.shape[1]}]: the cohorts must have the same features")
            if not bool(torch.isfinite(t).all().item()):
                raise ValueError(f"{name} holds non-finite values")
        if tr.shape[0] == 0 or (ho is not None and ho.shape[0] == 0):
            raise ValueError("the real cohorts must not be empty")
        rows = sharded_nearest_records(self.comm, self.k, tr, sy, ho)
        summary = self._agree(privacy_summary(rows))
        return (summary, rows) if return_rows else summary

    # -- diversity: precision / recall / density / coverage (no counterpart in the reference) ------
    def fidelity_diversity(self, real, synthetic, k: int = 5, return_rows: bool = False):
        """``prdc_precision``, ``prdc_recall``, ``prdc_density``, ``prdc_coverage`` and ``prdc_k`` of ``prdc_summary``: how much of
        the synthetic cohort lies where real patients are (precision, density) and how much of the real cohort the synthetic one
        reaches (recall, coverage) -- a collapsed sampler keeps the first pair and loses the second.  Four passes over distance
        rectangles that are never stored: the k-th-neighbour radius of every real and of every synthetic row inside its own cohort
        (``DeviceKernels.knn``, the row itself excluded), then the two count passes (``DeviceKernels.ball_counts``).  Distances
        are plain Euclidean over the columns as given -- callers scale their inputs.  The counts compare the fp32 expanded form
        with the recomputed radii, so a row exactly AT a radius may count either way.  1 <= k <= 16 and
        both cohorts need more than k rows.  ``return_rows=True`` also returns the per-row arrays (the three of ``prdc_summary``
        plus ``real_radius`` and ``synth_radius``, float64 distances).  Not available on a ``sharded=True`` validator."""
        if self.sharded:
            raise NotImplementedError("fidelity_diversity is not implemented for a sharded validator: the synthetic cohort's own "
                                      "k-th-neighbour radii need every synthetic row against every other (a ring exchange)")
        k = int(k)
        if not 1 <= k <= 16:
            raise ValueError("k must lie in [1, 16]")
        shapes = [tuple(a.shape) if hasattr(a, "shape") else np.shape(a) for a in (real, synthetic)]      # before anything moves
        for name, shp in zip(("real", "synthetic"), shapes):
            if len(shp) != 2 or shp[1] != shapes[0][-1]:
                raise ValueError(f"{name} must be [rows, features] and the cohorts must have the same features, got {shp}")
            if shp[0] <= k:
                raise ValueError(f"{name} has {shp[0]} rows: a k-th-neighbour radius needs more than k = {k}")
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        for name, t in (("real", x), ("synthetic", y)):
            if not bool(torch.isfinite(t).all().item()):
                raise ValueError(f"{name} holds non-finite values")
        r2 = []
        for t in (x, y):
            own = torch.arange(t.shape[0], dtype=torch.int32, device=t.device)
            r2.append(self.k.knn(t, t, k, own)[0][:, k - 1].contiguous())        # the recomputed d2 of the k-th neighbour
        in_real, _ = self.k.ball_counts(y, x, r2_ref=r2[0])
        in_synth, cover = self.k.ball_counts(x, y, r2_ref=r2[1], r2_query=r2[0])
        rows = {"synth_in_real_balls": in_real.cpu().numpy().astype(np.int64),
                "real_in_synth_balls": in_synth.cpu().numpy().astype(np.int64),
                "real_ball_synth": cover.cpu().numpy().astype(np.int64),
                "real_radius": np.sqrt(r2[0].cpu().numpy().astype(np.float64)),
                "synth_radius": np.sqrt(r2[1].cpu().numpy().astype(np.float64))}
        summary = prdc_summary(rows, k)
        return (summary, rows) if return_rows else summary

    # -- second-order structure: correlation matrices and the Frechet distance (no counterpart in the reference)
    def correlation_fidelity(self, real, synthetic, blocks=None, strong: float = 0.3, frechet: bool = False, return_matrices: bool = False):
        """How well ``synthetic`` keeps ``real``'s correlation structure: the ``corr_*`` keys of ``corr_summary`` over all pairs of
        columns (Pearson correlations of both cohorts from ``DeviceKernels.centered_gram``, compared on the device by
        ``DeviceKernels.corr_compare``; neither correlation matrix is stored).  ``blocks``: an ordered ``{name: width}`` mapping that
        splits the columns, for per-block-pair figures; ``strong``: |r_real| from which a pair counts as strongly correlated.
        ``frechet=True`` adds ``frechet_distance``'s keys from the means and G / (n - 1) of both cohorts -- two D x D symmetric
        eigen-decompositions on the host (seconds at D = 2000, most of a minute at D = 5000), hence off by default.  On a
        ``sharded=True`` validator ``synthetic`` is this rank's row shard and the real cohort is replicated.
        ``return_matrices=True`` also returns a dictionary with the device Gram matrices, the means, the row counts and the raw
        sums."""
        shapes = [tuple(a.shape) if hasattr(a, "shape") else np.shape(a) for a in (real, synthetic)]      # before anything moves
        for name, shp in zip(("real", "synthetic"), shapes):
            if len(shp) != 2 or shp[1] != shapes[0][-1] or shp[1] < 1:
                raise ValueError(f"{name} must be [rows, features] and the cohorts must have the same features, got {shp}")
            if shp[0] < 2 and not (self.comm.on and name == "synthetic"):
                raise ValueError(f"{name} has {shp[0]} rows: a correlation needs at least 2")
        bounds, names = corr_block_bounds(blocks, shapes[0][1])
        strong = float(strong)
        if not strong >= 0.0:
            raise ValueError("strong must be a non-negative threshold")
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        for name, t in (("real", x), ("synthetic", y)):
            if not bool(torch.isfinite(t).all().item()):
                raise ValueError(f"{name} holds non-finite values")
        n_r, mu_r, g_r = sharded_centered_gram(self._one, self.k, x)
        n_s, mu_s, g_s = sharded_centered_gram(self.comm, self.k, y)
        if n_s < 2:
            raise ValueError(f"synthetic has {n_s} rows: a correlation needs at least 2")
        stats = self.k.corr_compare(g_r, g_s, bounds, strong)
        summary = corr_summary(stats, bounds, names)
        if frechet:
            summary.update(frechet_distance(mu_r, (g_r / (n_r - 1)).cpu().numpy(), mu_s, (g_s / (n_s - 1)).cpu().numpy()))
        summary = self._agree(summary)
        if return_matrices:
            return summary, {"real_gram": g_r, "synth_gram": g_s, "real_mean": mu_r, "synth_mean": mu_s, "real_rows": n_r,
                             "synth_rows": n_s, "stats": stats, "bounds": bounds, "names": names}
        return summary

    # -- first-order structure: every feature's marginal (no counterpart in the reference) --------------------
    def marginal_fidelity(self, real, synthetic, blocks=None, return_rows: bool = False, chunk_cols: int = 0):
        """How well ``synthetic`` keeps each of ``real``'s D marginals: the ``marginal_*`` keys of ``marginal_summary`` -- per-feature
        two-sample KS distance, Wasserstein-1 distance in units of the real column's standard deviation, and the share of synthetic
        values outside the real column's observed range -- over ALL columns (``DeviceKernels.marginals``: a transposing gather, the
        segmented sort and one statistics pass, a chunk of columns at a time), where ``statistical_tests`` looks at the first 100.
        Effect sizes only, NO p-values: at these cohort sizes every feature is significant, ``kstwo.sf`` costs 8 ms per feature, and
        the report is there to say WHICH feature is off and by how much.  ``blocks``: an ordered ``{name: width}`` mapping that splits
        the columns, as in ``correlation_fidelity``, for per-block figures.  On a ``sharded=True`` validator ``synthetic`` is this
        rank's row shard and the real cohort is replicated.  ``return_rows=True`` also returns the per-feature arrays (``ks``,
        ``w1``, ``w1_scaled`` -- NaN for a constant feature --, ``below``, ``above``, ``ks_dmax``, ``ks_dmin``, ``real_sd``, the row
        counts) and ``worst_ks``, the indices of the ten features with the largest KS distance, worst first."""
        shapes = [tuple(a.shape) if hasattr(a, "shape") else np.shape(a) for a in (real, synthetic)]      # before anything moves
        for name, shp in zip(("real", "synthetic"), shapes):
            if len(shp) != 2 or shp[1] != shapes[0][-1] or shp[1] < 1:
                raise ValueError(f"{name} must be [rows, features] and the cohorts must have the same features, got {shp}")
            if shp[0] < 1 and not (self.comm.on and name == "synthetic"):
                raise ValueError(f"{name} has no rows")
        bounds, names = corr_block_bounds(blocks, shapes[0][1])
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        for name, t in (("real", x), ("synthetic", y)):
            if not bool(torch.isfinite(t).all().item()):
                raise ValueError(f"{name} holds non-finite values")
        rows = sharded_marginals(self.comm, self.k, x, y, chunk_cols)
        rows["real_sd"] = real_sample_sd(self.k, x)
        summary, rows = self._agree((marginal_summary(rows, bounds, names), rows))
        if not return_rows:
            return summary
        ks = marginal_ks(rows)
        with np.errstate(divide="ignore", invalid="ignore"):
            scaled = np.where(rows["real_sd"] > 0, rows["w1"] / rows["real_sd"], np.nan)
        rows.update(ks=ks, w1_scaled=scaled, worst_ks=np.argsort(-ks, kind="stable")[:10], bounds=bounds, names=names)
        return summary, rows

    # -- differential signal: per-feature rank statistics of two groups inside each cohort -------------------
    def differential_fidelity(self, real, real_cond, synthetic, synth_cond, names=None, blocks=None, alpha: float = 0.05,
                              top_k: int = 50, return_rows: bool = False):
        """Do the features that separate two groups of real patients separate them in ``synthetic`` too, in the same direction and by
        the same amount?  Every column of the condition matrices is one contrast: a column whose values all lie in {0, 1} in both
        cohorts is used as it is (1 a case, 0 a control); any other column is split at the REAL cohort's median, and the SAME
        threshold is applied to the synthetic cohort (a case is a value above it).  Per contrast and cohort one
        ``DeviceKernels.group_ranks`` call gives every feature's Mann-Whitney U with mid-ranks for ties -- the statistic has to be
        rank-based: the expression block is zero-inflated --, its tie correction and the groups' moments; ``diffexp.group_statistics``
        turns them into AUC, rank-biserial effect, z, p, Benjamini-Hochberg q, mean difference, Welch t and Cohen's d, and
        ``diffexp.contrast_summary`` compares the cohorts.  Keys, per contrast ``de_<key>_<contrast>``: ``effect_pearson``,
        ``effect_spearman``, ``effect_slope`` (below 1 the signal is flattened, above 1 exaggerated), ``sign_agreement`` over the real
        hits (q < ``alpha``), ``real_hits``, ``synth_hits``, ``precision``, ``recall``, ``topk_jaccard`` (``top_k`` features by
        |effect|), ``false_signal_share``, ``max_abs_effect_gap``, ``max_gap_feature`` and, with ``blocks`` (an ordered
        ``{name: width}`` mapping, as in ``correlation_fidelity``), ``effect_pearson_<block>``; then ``de_<key>_mean`` over the
        contrasts, ``de_contrasts`` and ``de_skipped``: a contrast with an empty group in either cohort is skipped and counted there.
        ``names``: one per condition column (default: the columns of ``real_cond``, else c0, c1, ...).  ``return_rows=True`` also
        returns, per contrast, both cohorts' per-feature arrays and the threshold.  At most 2^20 rows per cohort.  On a
        ``sharded=True`` validator the method raises a ValueError: the pairs of a U statistic couple rows across shards."""
        if self.sharded:
            raise ValueError("differential_fidelity is not available on a sharded validator: a U statistic counts pairs of rows, "
                             "which couples the rows of different shards")
        if names is None:
            cols = getattr(real_cond, "columns", None)
            names = [str(c) for c in cols] if cols is not None else None
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        cs = [np.asarray(_host(a), dtype=np.float64) for a in (real_cond, synth_cond)]
        cs = [c.reshape(-1, 1) if c.ndim == 1 else c for c in cs]
        K = cs[0].shape[1] if cs[0].ndim == 2 else 0
        if names is None:
            names = [f"c{j}" for j in range(K)]
        names = [str(v) for v in names]
        if K < 1 or len(names) != K or len(set(names)) != K or "mean" in names:
            raise ValueError("one distinct name per condition column (none of them 'mean'), and at least one condition")
        for label, t, c in zip(("real", "synthetic"), (x, y), cs):
            if t.dim() != 2 or t.shape[1] != x.shape[1] or t.shape[1] < 1 or t.shape[0] < 1:
                raise ValueError(f"{label} must be [rows >= 1, {x.shape[1]}]: the cohorts must have the same features")
            if c.ndim != 2 or c.shape != (t.shape[0], K):
                raise ValueError(f"the conditions of {label} must be [{t.shape[0]}, {K}], got {c.shape}")
            if not (bool(torch.isfinite(t).all().item()) and np.isfinite(c).all()):
                raise ValueError(f"{label} holds non-finite values")
        if not 0.0 < float(alpha) <= 1.0 or int(top_k) < 1:
            raise ValueError("alpha must lie in (0, 1] and top_k must be at least 1")
        bounds, block_names = corr_block_bounds(blocks, int(x.shape[1]))
        summary, rows = DE.differential_metrics(self.k, x, cs[0], y, cs[1], names, bounds, block_names, float(alpha), int(top_k))
        return (summary, rows) if return_rows else summary

    # -- counterfactual patients against the real cohort's own contrast --------------------------------------
    def counterfactual_consistency(self, original, counterfactual, real, real_cond, contrast, names=None, blocks=None,
                                   alpha: float = 0.05):
        """Does a set of counterfactuals (``SyntheticPatientGenerator.counterfactual``: row r of ``counterfactual`` is row r of
        ``original`` under the other condition) move the features the way the real cohort's own two groups differ?  ``contrast`` names
        the condition column (a name of ``names`` / of ``real_cond``'s columns, or an index) that was changed, split as
        ``differential_fidelity`` splits it: the counterfactuals are taken to move control rows (0, or at or below the real median)
        to the case side, so the reference is the real cases' mean minus the real controls'.  Both are in units of the real column's
        standard deviation (ddof = 1; a constant real column counts as 0 in both):

          ``cf_effect_pearson``, ``cf_effect_slope``   over the features, of the mean paired shift against the real mean difference
                                                       (``diffexp.contrast_summary``; slope below 1: the edit under-shoots)
          ``cf_sign_agreement``    over the real hits (Mann-Whitney q < ``alpha``), the share whose shift has the real difference's sign
          ``cf_real_hits``         their number
          ``cf_mean_abs_shift``    the mean over the features of |mean paired shift| / sd
          ``cf_rows_changed_mutation_share``   with ``blocks`` naming a ``mutations`` block: the share of rows in which any mutation,
                                               read at 0.5, differs between the pair; NaN without one

        Host composition over ``DeviceKernels.group_ranks`` and ``col_centered_moments``; no sharded form (as ``differential_fidelity``)."""
        if self.sharded:
            raise ValueError("counterfactual_consistency is not available on a sharded validator: it reads the real cohort's U statistics")
        if names is None:
            cols = getattr(real_cond, "columns", None)
            names = [str(c) for c in cols] if cols is not None else None
        x, o, c = _dev(real, self.device), _dev(original, self.device), _dev(counterfactual, self.device)
        rc = np.asarray(_host(real_cond), dtype=np.float64)
        rc = rc.reshape(-1, 1) if rc.ndim == 1 else rc
        D = int(x.shape[1]) if x.dim() == 2 else 0
        if x.dim() != 2 or D < 1 or x.shape[0] < 2 or rc.shape[0] != x.shape[0]:
            raise ValueError("real must be [rows >= 2, D] with one condition row per real row")
        if o.dim() != 2 or o.shape != c.shape or o.shape[1] != D or o.shape[0] < 1:
            raise ValueError(f"original and counterfactual must be paired [rows >= 1, {D}] arrays")
        if not (bool(torch.isfinite(x).all().item()) and bool(torch.isfinite(o).all().item()) and bool(torch.isfinite(c).all().item())
                and np.isfinite(rc).all()):
            raise ValueError("counterfactual_consistency: non-finite values")
        if isinstance(contrast, str):
            if names is None or contrast not in [str(v) for v in names]:
                raise ValueError(f"contrast {contrast!r} is not among the condition names {names}")
            j = [str(v) for v in names].index(contrast)
        else:
            j = int(contrast)
        if not 0 <= j < rc.shape[1]:
            raise ValueError(f"contrast index {j} outside the {rc.shape[1]} condition columns")
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError("alpha must lie in (0, 1]")
        bounds, block_names = corr_block_bounds(blocks, D)
        labels, _, _ = DE.contrast_labels(rc[:, j], rc[:, j])
        if min(int((labels == 1).sum()), int((labels == 0).sum())) < 1:
            raise ValueError("the contrast has an empty group in the real cohort")
        stat = DE.cohort_statistics(self.k, x, labels)
        n_real, n = int(x.shape[0]), int(o.shape[0])
        s0, _ = self.k.col_centered_moments(x)
        center = (np.asarray(s0, dtype=np.float64) / n_real).astype(np.float32)
        s1, q1 = self.k.col_centered_moments(x, center)
        sd = np.sqrt(np.maximum(q1 - s1 * s1 / n_real, 0.0) / (n_real - 1.0))
        ds, _ = self.k.col_centered_moments(c - o)
        with np.errstate(divide="ignore", invalid="ignore"):
            shift = np.where(sd > 0, (ds / n) / sd, 0.0)
            ref = np.where(sd > 0, stat["mean_diff"] / sd, 0.0)
        one = DE.contrast_summary({"effect": ref, "q": stat["q"]}, {"effect": shift, "q": np.ones(D)}, float(alpha), 1)
        out = {"cf_effect_pearson": one["effect_pearson"], "cf_effect_slope": one["effect_slope"], "cf_sign_agreement": one["sign_agreement"],
               "cf_real_hits": one["real_hits"], "cf_mean_abs_shift": float(np.abs(shift).mean()),
               "cf_rows_changed_mutation_share": float("nan")}
        if "mutations" in block_names:
            b = block_names.index("mutations")
            lo, hi = bounds[b], bounds[b + 1]
            out["cf_rows_changed_mutation_share"] = float(((o[:, lo:hi] > 0.5) != (c[:, lo:hi] > 0.5)).any(dim=1).double().mean().item())
        return out

    # -- prognostic genes: one Cox model per feature and cohort ---------------------------------------------
    def prognostic_fidelity(self, real, real_surv, synthetic, synth_surv, blocks=None, alpha: float = 0.05, top_k: int = 50,
                            mle: bool = True, return_rows: bool = False):
        """Do the features that are prognostic among the real patients stay prognostic among the synthetic ones, in the same
        direction and by the same hazard ratio?  ``*_surv`` is [rows, 2] = (time, event) as in ``survival_utility``: censoring is
        respected -- a patient censored at 300 days is at risk until then and never a short survivor, unlike the median split
        ``differential_fidelity`` would make of the time.  Per cohort one univariate Cox screen over every feature
        (``survival.cox_screen`` over ``DeviceKernels.cox_score``: Breslow ties, a score test at 0 -- the log-rank test of the
        feature -- with Benjamini-Hochberg q, and with ``mle`` the per-feature maximum-likelihood log hazard ratio by Newton
        iterations, each two reads of the cohort; ``mle=False``: the one-step estimate score / info, two reads in all).  BOTH cohorts
        are standardised with the REAL cohort's column mean and sample standard deviation, so an effect is a log hazard ratio per
        real standard deviation in either cohort.  A constant real column is left out and counted.

        Keys: ``prog_<key>`` for every key of ``diffexp.contrast_summary`` over the two screens' ``effect`` and ``q`` (a hit is
        q < ``alpha``; ``prog_effect_slope`` below 1: the prognostic signal is flattened; ``prog_max_gap_feature`` is a column index
        of ``real``; with ``blocks``, an ordered ``{name: width}`` mapping, ``prog_effect_pearson_<block>``), ``prog_features``,
        ``prog_constant_features``, ``prog_not_converged_real`` / ``_synth`` (features whose fit hit the clamp, ran out of
        iterations or has no information in that cohort; such a synthetic feature counts as effect 0, q 1),
        ``prog_events_real`` / ``_synth`` and ``prog_max_abs_z_real`` / ``_synth``.  ``return_rows=True`` also returns both
        screens' per-feature arrays.  An all-censored cohort raises a ValueError naming it.  At most 8192 features.  On a
        ``sharded=True`` validator the method raises a ValueError: a risk set couples the rows of different shards."""
        if self.sharded:
            raise ValueError("prognostic_fidelity is not available on a sharded validator: the risk set of a patient holds rows of "
                             "every shard")
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        for label, t in (("real", x), ("synthetic", y)):
            if t.dim() != 2 or t.shape[1] != x.shape[1] or t.shape[1] < 1 or t.shape[0] < 2:
                raise ValueError(f"{label} must be [rows >= 2, {x.shape[1]}]: the cohorts must have the same features")
            if not bool(torch.isfinite(t).all().item()):
                raise ValueError(f"{label} holds non-finite values")
        if not 0.0 < float(alpha) <= 1.0 or int(top_k) < 1:
            raise ValueError("alpha must lie in (0, 1] and top_k must be at least 1")
        bounds, block_names = corr_block_bounds(blocks, int(x.shape[1]))
        summary, rows = prognostic_metrics(self.k, x, np.asarray(_host(real_surv), dtype=np.float64), y,
                                           np.asarray(_host(synth_surv), dtype=np.float64), bounds, block_names, float(alpha),
                                           int(top_k), bool(mle))
        return (summary, rows) if return_rows else summary

    # -- pathway enrichment: preranked GSEA with a device permutation null ------------------------------------
    def enrichment_fidelity(self, real, real_cond, synthetic, synth_cond, gene_sets, names=None, weight: float = 1.0,
                            permutations: int = 1000, min_size: int = 5, max_size: int = 500, alpha: float = 0.05, seed: int = 0,
                            return_rows: bool = False):
        """Is a gene set up or down between two groups of synthetic patients as it is between the real ones?  Preranked gene-set
        enrichment analysis per cohort and contrast (the contrasts as in ``differential_fidelity``: every column of the condition
        matrices, a 0/1 column as it is, any other split at the REAL cohort's median): the genes -- the columns of ``real`` and
        ``synthetic`` -- are ranked by the Mann-Whitney z of ``diffexp.cohort_statistics``, a position weighs |z| ** ``weight``
        (0: the classic Kolmogorov-Smirnov form), and one ``DeviceKernels.gsea`` call gives every set's enrichment score under the
        identity and under ``permutations`` gene-label permutations shared by all sets (``seed``); ``enrichment.py`` turns them into
        ES, NES, p, Benjamini-Hochberg q and the leading-edge size and compares the cohorts.  ``gene_sets``: an ordered
        ``{name: column indices}`` mapping, or a [D, S] 0/1 matrix or DataFrame whose columns name the sets; members are
        de-duplicated, and a set with fewer than ``min_size`` or more than min(``max_size``, 1024, D - 1) members is dropped and
        counted in ``gsea_sets_skipped`` (no set left: a ValueError).  Keys, per contrast ``gsea_<key>_<contrast>``:
        ``nes_pearson``, ``nes_spearman``, ``nes_slope``, ``sign_agreement`` over the real hits (q < ``alpha``), ``real_hits``,
        ``synth_hits``, ``precision``, ``recall``, ``false_signal_share``, ``max_abs_nes_gap``, ``max_gap_set`` (an index into the
        kept sets); then ``gsea_<key>_mean`` over the contrasts, ``gsea_contrasts``, ``gsea_skipped``, ``gsea_sets`` and
        ``gsea_sets_skipped``.  ``return_rows=True`` also returns, per contrast, both cohorts' per-set arrays, plus ``sets``, the kept
        sets' names.  At most 32768 columns.  On a ``sharded=True`` validator the method raises a ValueError: the U statistic
        underneath couples rows across shards."""
        if self.sharded:
            raise ValueError("enrichment_fidelity is not available on a sharded validator: the U statistic that ranks the genes "
                             "counts pairs of rows, which couples the rows of different shards")
        if names is None:
            cols = getattr(real_cond, "columns", None)
            names = [str(c) for c in cols] if cols is not None else None
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        cs = [np.asarray(_host(a), dtype=np.float64) for a in (real_cond, synth_cond)]
        cs = [c.reshape(-1, 1) if c.ndim == 1 else c for c in cs]
        K = cs[0].shape[1] if cs[0].ndim == 2 else 0
        if names is None:
            names = [f"c{j}" for j in range(K)]
        names = [str(v) for v in names]
        if K < 1 or len(names) != K or len(set(names)) != K or "mean" in names:
            raise ValueError("one distinct name per condition column (none of them 'mean'), and at least one condition")
        for label, t, c in zip(("real", "synthetic"), (x, y), cs):
            if t.dim() != 2 or t.shape[1] != x.shape[1] or t.shape[1] < 2 or t.shape[0] < 1:
                raise ValueError(f"{label} must be [rows >= 1, {x.shape[1]}]: the cohorts must have the same features, two at least")
            if c.ndim != 2 or c.shape != (t.shape[0], K):
                raise ValueError(f"the conditions of {label} must be [{t.shape[0]}, {K}], got {c.shape}")
            if not (bool(torch.isfinite(t).all().item()) and np.isfinite(c).all()):
                raise ValueError(f"{label} holds non-finite values")
        if not 0.0 < float(alpha) <= 1.0 or int(permutations) < 0 or not 0.0 <= float(weight) <= 16.0:
            raise ValueError("alpha must lie in (0, 1], permutations must not be negative and weight must lie in [0, 16]")
        if x.shape[1] > 32768:
            raise ValueError("enrichment_fidelity ranks at most 32768 columns")
        set_names, sets, dropped = EN.select_sets(gene_sets, int(x.shape[1]), int(min_size), int(max_size))
        if not sets:
            raise ValueError("no gene set is left between min_size and max_size")
        summary, rows = EN.enrichment_metrics(self.k, x, cs[0], y, cs[1], names, sets, float(weight), int(permutations), float(alpha),
                                              int(seed), dropped)
        rows["sets"] = set_names
        return (summary, rows) if return_rows else summary

    # -- pathway consistency: the generated pathway block against the scores of the generated expression -----
    def pathway_consistency(self, synth_expression, synth_pathways, gene_sets, real_expression, real_pathways=None,
                            method: str = "mean", alpha: float = 0.25, return_rows: bool = False, min_genes: int = 5):
        """Does a generated patient's pathway block agree with the pathway scores of that same patient's generated expression?  In
        the real cohort the block is a function of the expression; shuffling the pathway rows among the synthetic patients leaves
        every marginal, the MMD and every per-gene contrast as they were -- this check is the one that moves.  A
        ``pathways.PathwayScorer`` (``method``: ``mean``, ``zscore`` or ``ssgsea`` with the exponent ``alpha``; ``min_genes``) is
        fitted on ``real_expression``; z = the standardised scores of ``synth_expression`` (``DeviceKernels.pathway_scores``, then
        (p - mean) / (sd + 1e-8) with the REAL cohort's figures, as ``prepare_data`` standardises), g = ``synth_pathways``; frames
        are matched by column name, a bare pathway matrix must hold exactly the kept sets.  ``gene_sets``: a name -> gene symbols
        mapping, a name -> column indices mapping or a genes x sets 0/1 DataFrame.  Per pathway, over the rows where z and g are
        finite (``DeviceKernels.pathway_agreement``): Pearson r(g, z), ``rmse`` = sqrt(mean (g - z)^2) -- in real-cohort sd units
        by construction --, ``bias`` = mean g - mean z and ``sd_ratio`` = sd g / sd z.  Keys: ``pwc_pearson_mean`` / ``_min`` /
        ``_min_pathway``, ``pwc_rmse_mean`` / ``_max`` / ``_max_pathway``, ``pwc_abs_bias_mean``, ``pwc_sd_ratio_mean``, ``pwc_r2``
        (pooled: 1 - sum (g - z)^2 / sum (z - mean z)^2), ``pwc_pathways``, ``pwc_pathways_skipped``, ``pwc_constant`` (pathways
        whose z or g is constant: no r) and ``pwc_rows_nonfinite`` (the left-out rows, added over the pathways).  With
        ``real_pathways`` the same figures of the real cohort as ``pwc_real_*``: r = 1 and rmse = 0 when the block came from this
        scorer -- the baseline for a block that another method made.  ``return_rows=True`` also returns the per-pathway arrays.
        On a ``sharded=True`` validator the synthetic arguments are this rank's rows: rows are independent, the six sums add
        across ranks, the fit is on the replicated real cohort."""
        summary, rows = PW.pathway_consistency(self.comm, self.k, self.device, synth_expression, synth_pathways, gene_sets,
                                               real_expression, real_pathways, method=method, alpha=float(alpha), min_genes=int(min_genes))
        summary, rows = self._agree((summary, rows))
        return (summary, rows) if return_rows else summary

    # -- downstream utility: TSTR and the classifier two-sample test (no counterpart in the reference) ------
    def downstream_utility(self, real_train, real_train_cond, synthetic, synth_cond, real_test, real_test_cond, names=None,
                           l2: float = 1e-2, max_iter: int = 200, tol: float = 1e-5) -> Dict[str, float]:
        """Train on synthetic, test on real: does the synthetic cohort carry the relation between the features and the conditions
        the patients were generated under?  Each condition column is one head of an L2-regularised linear model of the features
        (logistic where its values all lie in {0, 1} over the three cohorts, else least squares on the target standardised by the
        training cohort), fitted once on ``synthetic`` / ``synth_cond`` (TSTR) and once on ``real_train`` / ``real_train_cond`` (TRTR)
        -- features standardised by the cohort the fit trains on --, and both fits score ``real_test``.  Keys, per head:
        ``utility_tstr_auc_<name>``, ``utility_trtr_auc_<name>``, ``utility_auc_gap_<name>`` (TRTR - TSTR) or the same with ``r2``;
        and ``utility_gap_mean``.  ``names``: one per condition column (default: the columns of ``real_train_cond``, else c0, c1,
        ...).  Every iteration of a fit is one pass of ``DeviceKernels.glm_eval`` over the cohort, four heads at a time.  A logistic
        head with a single class in a training or the test cohort raises a ValueError naming the column.  On a ``sharded=True``
        validator ``synthetic`` and ``synth_cond`` are this rank's row shard; the real cohorts are replicated."""
        if names is None:
            cols = getattr(real_train_cond, "columns", None)
            names = [str(c) for c in cols] if cols is not None else None
        xs = [_dev(a, self.device) for a in (real_train, synthetic, real_test)]
        cs = [np.asarray(_host(a), dtype=np.float64) for a in (real_train_cond, synth_cond, real_test_cond)]
        cs = [c.reshape(-1, 1) if c.ndim == 1 else c for c in cs]
        K = cs[0].shape[1]
        if names is None:
            names = [f"c{j}" for j in range(K)]
        names = [str(v) for v in names]
        if K < 1 or len(names) != K:
            raise ValueError("one name per condition column, and at least one condition")
        for label, x, c in zip(("real_train", "synthetic", "real_test"), xs, cs):
            if x.dim() != 2 or x.shape[1] != xs[0].shape[1] or x.shape[1] < 1:
                raise ValueError(f"{label} must be [rows, {xs[0].shape[1]}]: the cohorts must have the same features")
            if c.ndim != 2 or c.shape != (x.shape[0], K):
                raise ValueError(f"the conditions of {label} must be [{x.shape[0]}, {K}], got {c.shape}")
            if not (bool(torch.isfinite(x).all().item()) and np.isfinite(c).all()):
                raise ValueError(f"{label} holds non-finite values")
            if x.shape[0] < 2 and not (self.comm.on and label == "synthetic"):
                raise ValueError(f"{label} has {x.shape[0]} rows: a fit needs at least 2")
        return self._agree(utility_metrics(self.comm, self.k, xs[0], cs[0], xs[1], cs[1], xs[2], cs[2], names, l2=float(l2),
                                           max_iter=int(max_iter), tol=float(tol)))

    def discriminator_test(self, real, synthetic, test_fraction: float = 0.3, seed: int = 0, l2: float = 1e-2, max_iter: int = 200,
                           tol: float = 1e-5) -> Dict[str, float]:
        """The classifier two-sample test: can an L2-regularised logistic model of the features tell real (0) from synthetic (1)?
        Each cohort is split by a seeded permutation, the model is fitted on the training parts -- features standardised by the
        two together, row weights that give both classes the same total weight, the two cohorts evaluated as two
        ``DeviceKernels.glm_eval`` calls whose sums are added, never concatenated -- and the held-out rows give ``c2st_auc``,
        ``c2st_accuracy`` (balanced) and ``c2st_pmse``, the mean of (p - 1/2)^2.  0.5, 0.5 and 0 mean the cohorts are
        indistinguishable; 1, 1 and 1/4 that every held-out row is told apart with certainty.  On a ``sharded=True`` validator
        ``synthetic`` is this rank's row shard."""
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        for label, t in (("real", x), ("synthetic", y)):
            if t.dim() != 2 or t.shape[1] != x.shape[1] or t.shape[1] < 1:
                raise ValueError(f"{label} must be [rows, {x.shape[1]}]: the cohorts must have the same features")
            if not bool(torch.isfinite(t).all().item()):
                raise ValueError(f"{label} holds non-finite values")
        return self._agree(c2st_metrics(self.comm, self.k, x, y, test_fraction=float(test_fraction), seed=int(seed), l2=float(l2),
                                        max_iter=int(max_iter), tol=float(tol)))

    # -- survival utility: Cox fits on synthetic and on real patients, concordance on held-out real ones ------
    def survival_utility(self, real_train, real_train_surv, synthetic, synth_surv, real_test, real_test_surv, l2: float = 1e-2,
                         max_iter: int = 200, tol: float = 1e-5) -> Dict[str, float]:
        """Train on synthetic, test on real, for the survival conditions: does a proportional-hazards model trained on the synthetic
        cohort order held-out real patients by risk as well as one trained on real patients?  Each ``*_surv`` is [rows, 2] =
        (follow-up time, event flag: 1 an event, 0 a censoring), so a censored patient enters every risk set up to their time and no
        event term -- unlike ``downstream_utility``, which would regress on the time as if it were an event.  One L2-regularised Cox
        fit (Breslow ties, ``survival.fit_cox`` over ``DeviceKernels.cox_eval``: two reads of the cohort per iteration) on
        ``synthetic`` (TSTR) and one on ``real_train`` (TRTR), features standardised by the cohort the fit trains on; both score
        ``real_test`` and Harrell's C is counted exactly on the device (``DeviceKernels.concordance``).  Keys:
        ``survival_tstr_cindex``, ``survival_trtr_cindex``, ``survival_cindex_gap`` (TRTR - TSTR), ``survival_coef_cosine`` (between
        the two coefficient vectors in raw-feature units), ``survival_comparable_pairs`` and ``survival_event_share_real_train`` /
        ``_synthetic`` / ``_real_test``.  A cohort without an event, or a test cohort without a comparable pair, raises a ValueError
        naming the cohort; so does non-finite input.  Times are compared as fp32 values.  Not available on a ``sharded=True``
        validator."""
        if self.sharded:
            raise NotImplementedError("survival_utility is not implemented for a sharded validator: the risk set of a patient holds "
                                      "every patient with a later time, so the partial likelihood couples rows across shards")
        xs = [_dev(a, self.device) for a in (real_train, synthetic, real_test)]
        ss = [np.asarray(_host(a), dtype=np.float64) for a in (real_train_surv, synth_surv, real_test_surv)]
        for label, x, s in zip(("real_train", "synthetic", "real_test"), xs, ss):
            if x.dim() != 2 or x.shape[1] != xs[0].shape[1] or x.shape[1] < 1:
                raise ValueError(f"{label} must be [rows, {xs[0].shape[1]}]: the cohorts must have the same features")
            if s.ndim != 2 or s.shape != (x.shape[0], 2):
                raise ValueError(f"the survival columns of {label} must be [{x.shape[0]}, 2] = (time, event), got {s.shape}")
            if not (bool(torch.isfinite(x).all().item()) and np.isfinite(s).all()):
                raise ValueError(f"{label} holds non-finite values")
            if x.shape[0] < 2:
                raise ValueError(f"{label} has {x.shape[0]} rows: a fit needs at least 2")
        return survival_metrics(self.k, xs[0], ss[0], xs[1], ss[1], xs[2], ss[2], l2=float(l2), max_iter=int(max_iter), tol=float(tol))

    # -- subtype structure: k-means on the real cohort, the synthetic rows assigned to its centroids ------
    def subtype_fidelity(self, real, synthetic, n_clusters: int = 4, *, conditions=None, names=None, seed: int = 0, n_init: int = 4,
                         max_iter: int = 100, return_rows: bool = False):
        """Does ``synthetic`` reproduce ``real``'s subtypes, and in the right proportions?  k-means (``cluster.kmeans``: k-means++,
        ``n_init`` restarts from ``seed``) is fitted on the real cohort after the fp32 column means of ``real`` are subtracted from
        both, the subtypes are numbered by descending real count, every synthetic row goes to its nearest centroid, and
        ``subtype_summary`` reports the ``subtype_*`` keys: shares, their Jensen-Shannon divergence and total-variation distance,
        missing subtypes, per-subtype dispersion ratios (collapse onto a centre) and centroid shifts.  ``conditions=(real_cond,
        synth_cond)`` adds ``subtype_condition_gap_<name>`` per condition column (``names``: default the columns of ``real_cond``,
        else c0, c1, ...).  Distances are plain Euclidean over the columns as given -- callers scale their inputs.
        ``return_rows=True`` also returns the sums behind the figures with the centroids, both label arrays and both d2 arrays.
        On a ``sharded=True`` validator ``synthetic`` (and ``synth_cond``) is this rank's row shard and the real cohort is
        replicated: the fit is local and identical on every rank, the synthetic sums are added over the ranks."""
        K = int(n_clusters)
        if not 1 <= K <= CL.MAX_CLUSTERS:
            raise ValueError(f"n_clusters must lie in [1, {CL.MAX_CLUSTERS}], got {K}")
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        for label, t in (("real", x), ("synthetic", y)):
            if t.dim() != 2 or t.shape[1] != x.shape[1] or t.shape[1] < 1:
                raise ValueError(f"{label} must be [rows, {x.shape[1]}]: the cohorts must have the same features")
            if not bool(torch.isfinite(t).all().item()):
                raise ValueError(f"{label} holds non-finite values")
        if x.shape[0] < K:
            raise ValueError(f"real has {x.shape[0]} rows: {K} subtypes need at least as many")
        if int(self.comm.sum(int(y.shape[0]))[0]) < 1:
            raise ValueError("synthetic has no rows")
        cond = None
        if conditions is not None:
            if not isinstance(conditions, (tuple, list)) or len(conditions) != 2:
                raise ValueError("conditions must be a (real_cond, synth_cond) pair")
            if names is None:
                cols = getattr(conditions[0], "columns", None)
                names = [str(c) for c in cols] if cols is not None else None
            cs = [_dev(c, self.device) for c in conditions]
            cs = [c.reshape(-1, 1) if c.dim() == 1 else c for c in cs]
            for label, c, t in zip(("real", "synthetic"), cs, (x, y)):
                if c.dim() != 2 or c.shape[0] != t.shape[0] or c.shape[1] != cs[0].shape[1] or c.shape[1] < 1:
                    raise ValueError(f"the conditions of {label} must be [{t.shape[0]}, {cs[0].shape[1]}], got {tuple(c.shape)}")
                if not bool(torch.isfinite(c).all().item()):
                    raise ValueError(f"the conditions of {label} hold non-finite values")
            names = [f"c{j}" for j in range(cs[0].shape[1])] if names is None else [str(v) for v in names]
            if len(names) != cs[0].shape[1]:
                raise ValueError("one name per condition column")
            cond = (cs[0].contiguous(), cs[1].contiguous())
        rows = CL.subtype_rows(self.comm, self.k, x, y, K, conditions=cond, names=names, seed=int(seed), n_init=int(n_init),
                               max_iter=int(max_iter))
        summary = self._agree(subtype_summary(rows))
        return (summary, rows) if return_rows else summary

    # -- low-dimensional structure: principal components by subspace iteration (no counterpart in the reference)
    def embedding_fidelity(self, real, synthetic, n_components: int = 10, standardize: bool = False, quantile: float = 0.99,
                           return_rows: bool = False, **pca_options):
        """Does ``synthetic`` live on ``real``'s low-dimensional structure?  A ``pca.DevicePCA`` (``n_components`` directions,
        ``standardize`` and ``pca_options`` -- oversample, max_iter, tol, seed -- as its constructor takes them) is fitted on each
        cohort, both cohorts are projected onto the REAL components about the real mean, and ``pca.embedding_summary`` reports the
        ``pca_*`` keys: per-axis variance ratios (a flattened axis is below 1), the mean shift, the Wasserstein-1 and KS distances
        of the scores (``pca_wasserstein_distance_mean`` is the reference's figure), the residual ratio and the share of synthetic
        rows farther from the real subspace than the ``quantile``-quantile of the real rows (variance spread off the manifold), and
        the cosines of the principal angles between the two fitted subspaces (a rotated leading subspace).  ``return_rows=True``
        also returns the fp32 scores of both cohorts (device tensors), the float64 residuals and both component matrices.  On a
        ``sharded=True`` validator ``synthetic`` is this rank's row shard and the real cohort is replicated: the synthetic fit goes
        through the communicator, scores and residuals are gathered before the marginals and the quantile count."""
        x, y = _dev(real, self.device), _dev(synthetic, self.device)
        for label, t in (("real", x), ("synthetic", y)):
            if t.dim() != 2 or t.shape[1] != x.shape[1] or t.shape[1] < 1:
                raise ValueError(f"{label} must be [rows, {x.shape[1]}]: the cohorts must have the same features")
            if not bool(torch.isfinite(t).all().item()):
                raise ValueError(f"{label} holds non-finite values")
        if x.shape[0] < 2 or int(self.comm.sum(int(y.shape[0]))[0]) < 2:
            raise ValueError("both cohorts need at least 2 rows")
        if not 0.0 <= float(quantile) <= 1.0:
            raise ValueError("quantile must lie in [0, 1]")
        rows = PC.embedding_rows(self.comm, self.k, x, y, int(n_components), bool(standardize), **pca_options)
        summary = self._agree(PC.embedding_summary(rows, float(quantile)))
        if not return_rows:
            return summary
        return summary, {"real_scores": rows["real_scores"], "synth_scores": rows["synth_scores"], "real_resid2": rows["real_resid2"],
                         "synth_resid2": rows["synth_resid2"], "real_components": rows["real"].components_,
                         "synth_components": rows["synth"].components_, "real_pca": rows["real"], "synth_pca": rows["synth"]}

    # -- privacy: membership inference on the per-record likelihood bound ---------------------
    def membership_audit(self, model, train, holdout, *, num_timesteps: int = 32, seed: int = 0) -> Dict[str, float]:
        """The loss-threshold membership-inference attack on a diffusion model: ``train`` and ``holdout`` are (data, conditions)
        pairs, both cohorts are scored with ``model.variational_bound`` (bits per feature, ``num_timesteps`` strided timesteps, the
        same ``seed``; holdout ids follow the train ids) and a lower score means "member".  Returns ``auc`` (Mann-Whitney by
        ranks, ties count half, on the host), ``tpr_at_1pct_fpr``, ``advantage`` (max over thresholds of TPR - FPR),
        ``mean_bpd_train`` and ``mean_bpd_holdout``.  0.5 / 0 / 0 is what a model that memorised nothing gives up to sampling
        noise.  A model that carries a feature transform (``model.feature_transform``) takes both cohorts in data units: they are
        mapped forward on the device first."""
        from . import likelihood as LK
        if hasattr(model, "_refuse_link"):
            model._refuse_link("membership_audit")      # it scores with variational_bound, which a linked model does not have
        scores = []
        offset = 0
        for name, cohort in (("train", train), ("holdout", holdout)):
            if not isinstance(cohort, (tuple, list)) or len(cohort) != 2:
                raise ValueError(f"{name} must be a (data, conditions) pair")
            data, cond = (_dev(v, self.device) for v in cohort)
            if data.dim() != 2 or data.shape[0] == 0:
                raise ValueError(f"{name} data must be [rows >= 1, features]")
            if getattr(model, "feature_transform", None) is not None:
                data = model.feature_transform.forward(data)        # cohorts come in data units; the bound is a model-space score
            out = model.variational_bound(data, cond, num_timesteps=num_timesteps, seed=seed, row_offset=offset)
            offset += data.shape[0]
            scores.append(out["bpd"].cpu().numpy())
        res = LK.membership_metrics(scores[0], scores[1])
        res["mean_bpd_train"] = float(scores[0].mean())
        res["mean_bpd_holdout"] = float(scores[1].mean())
        return res

    # -- utils/validation.py:27-121 ----------------------------------------------------------------
    def _column_sums(self, t: torch.Tensor) -> np.ndarray:
        return self.k.column_sums(t)

    def _gram(self, t: torch.Tensor, cols) -> np.ndarray:
        """Exact joint counts sum_r x[r][ci] x[r][cj] of 0/1 columns, 64 columns per device pass."""
        return self.k.gram(t, list(cols))

    @staticmethod
    def _chi2(n: int, n1: int, n2: int, n11: int) -> float:
        """chi2 of scipy.stats.chi2_contingency(pd.crosstab(a, b)) from the counts of two 0/1 columns (:98-108)."""
        from scipy import stats
        table = np.array([[n - n1 - n2 + n11, n2 - n11], [n1 - n11, n11]], dtype=np.int64)
        table = table[table.sum(1) > 0][:, table.sum(0) > 0]      # crosstab lists only the values that occur
        return float(stats.chi2_contingency(table)[0])

    def validate_mutation_cooccurrence(self, real_mutations, synthetic_mutations) -> Dict[str, float]:
        """real_mutations / synthetic_mutations: DataFrames of 0/1 columns named by gene."""
        logger.info("Validating mutation co-occurrence patterns...")
        results: Dict[str, float] = {}
        common = real_mutations.columns.intersection(synthetic_mutations.columns)
        r, s = _dev(real_mutations[common], self.device), _dev(synthetic_mutations[common], self.device)
        n_synth = int(self.comm.sum(s.shape[0])[0])
        pos = {g: i for i, g in enumerate(common)}
        real_freq, synth_freq = self._column_sums(r) / r.shape[0], self.comm.sum(self._column_sums(s)) / n_synth
        results["mutation_frequency_correlation"] = float(np.corrcoef(real_freq, synth_freq)[0, 1])
        logger.info(f"Mutation frequency correlation: {results['mutation_frequency_correlation']:.3f}")
        sfull = _dev(synthetic_mutations, self.device)
        spos = {g: i for i, g in enumerate(synthetic_mutations.columns)}
        drivers = [g for g in self.driver_genes if g in real_mutations.columns]
        if drivers:
            sfreq_all = self.comm.sum(self._column_sums(sfull)) / n_synth
            rd = np.array([float(real_mutations[g].mean()) for g in drivers])       # Series.mean() or a device vector's
            sd = np.array([sfreq_all[spos[g]] for g in drivers])       # KeyError if a driver gene is missing, as the reference
            results["driver_gene_frequency_diff"] = float(np.abs(rd - sd).mean())
            logger.info(f"Driver gene frequency difference: {results['driver_gene_frequency_diff']:.3f}")
        if self.mutually_exclusive_pairs:
            pairs = [(a, b) for a, b in self.mutually_exclusive_pairs if a in spos and b in spos]
            if pairs:
                violations = 0
                for a, b in pairs:                       # both-mutated count = off-diagonal of the 2-column Gram block
                    violations += int(round(self.comm.sum(self._gram(sfull, [spos[a], spos[b]]).ravel())[1]))
                results["mutual_exclusivity_violation_rate"] = violations / (n_synth * len(pairs))
                logger.info(f"Mutual exclusivity violation rate: {results['mutual_exclusivity_violation_rate']:.3f}")
        # pairwise chi-square on a random subset of at most 50 genes (np.random.choice, as the reference; rank 0 draws)
        sample_genes = self.comm.bcast_object(list(np.random.choice(common, size=min(50, len(common)), replace=False)))
        idx = [pos[g] for g in sample_genes]
        if len(idx) >= 2:
            gr = self._gram(r, idx)
            gs = self.comm.sum(self._gram(s, idx).ravel()).reshape(len(idx), len(idx))
            chi_r, chi_s = _chi2_pairs(r.shape[0], gr), _chi2_pairs(n_synth, gs)       # pairs i < j in row-major order, as the reference's loops
            results["cooccurrence_pattern_correlation"] = float(np.corrcoef(chi_r, chi_s)[0, 1])
            logger.info(f"Co-occurrence pattern correlation: {results['cooccurrence_pattern_correlation']:.3f}")
        return self._agree(results)

    # -- utils/validation.py:125-175 -------------------------------------------------------------
    def _mean_offdiag(self, data: torch.Tensor, cols, sharded: bool = False) -> float:
        return sharded_mean_offdiag(self.comm if sharded else self._one, self.k, data, list(cols))

    def validate_pathway_coherence(self, real_data, synthetic_data, pathway_gene_matrix) -> Dict[str, float]:
        """real_data / synthetic_data: DataFrames with gene columns; pathway_gene_matrix: genes x pathways 0/1."""
        logger.info("Validating pathway coherence...")
        col_of = {g: i for i, g in enumerate(real_data.columns)}
        syn_of = {g: i for i, g in enumerate(synthetic_data.columns)}
        r, s = _dev(real_data, self.device), _dev(synthetic_data, self.device)
        real_scores, synth_scores = [], []
        for pathway in pathway_gene_matrix.columns[:10]:
            genes = pathway_gene_matrix[pathway_gene_matrix[pathway] == 1].index
            genes = [g for g in genes if g in col_of]
            if len(genes) < 3:
                continue
            real_scores.append(self._mean_offdiag(r, [col_of[g] for g in genes]))
            synth_scores.append(self._mean_offdiag(s, [syn_of[g] for g in genes], sharded=True))
        results = {}
        if real_scores:
            results["real_pathway_coherence"] = float(np.mean(real_scores))
            results["synthetic_pathway_coherence"] = float(np.mean(synth_scores))
            results["pathway_coherence_correlation"] = float(np.corrcoef(real_scores, synth_scores)[0, 1])
        return self._agree(results)

    # -- utils/validation.py:177-223 -------------------------------------------------------------
    def validate_mutation_expression_correlation(self, mutations, expression, pathway_scores) -> Dict[str, float]:
        """All three arguments are synthetic data (row shards when the validator is sharded)."""
        logger.info("Validating mutation-expression correlations...")
        mut, pw = _dev(mutations, self.device), _dev(pathway_scores, self.device)
        violations = total = 0
        for rule in self.required_correlations:
            gene, pathway, expected = rule["mutation"], rule["pathway"], rule["direction"]
            if gene not in mutations.columns or pathway not in pathway_scores.columns:
                continue
            gi, pi = list(mutations.columns).index(gene), list(pathway_scores.columns).index(pathway)
            corr = sharded_pearson(self.comm, self.k, mut, gi, pw, pi)
            if (expected == "positive" and corr < 0) or (expected == "negative" and corr > 0):
                violations += 1
            total += 1
            logger.info(f"{gene} vs {pathway}: corr={corr:.3f} (expected: {expected})")
        return self._agree({"mutation_expression_violation_rate": violations / total} if total else {})

    # -- utils/validation.py:300-383 ---------------------------------------------------------------
    def validate_all(self, real_mutations, real_expression, real_pathways, synth_mutations, synth_expression, synth_pathways,
                     pathway_gene_matrix=None, privacy: bool = False, holdout=None, model=None, membership=None,
                     prdc: bool = False, prdc_k: int = 5, correlation: bool = False, frechet: bool = False,
                     corr_strong: float = 0.3, utility=None, c2st: bool = False, subtypes: Optional[int] = None,
                     subtype_conditions=None, survival=None, marginals: bool = False, differential=None,
                     differential_names=None, enrichment=None, enrichment_names=None,
                     enrichment_permutations: int = 1000, consistency: bool = False,
                     consistency_method: str = "mean", prognostic=None, embedding: bool = False,
                     embedding_components: int = 10) -> Dict[str, float]:
        """``embedding=True`` adds ``embedding_fidelity``'s ``pca_*`` keys on the combined matrices (``embedding_components``
        directions); with the default nothing changes.
        ``prognostic=(real_surv, synth_surv)`` adds ``prognostic_fidelity``'s ``prog_*`` keys on the combined matrices (blocks
        ``mutations`` / ``expression`` / ``pathways``; each ``*_surv`` is [rows, 2] = (time, event)); with the default None nothing
        changes.
        ``consistency=True`` adds ``pathway_consistency``'s ``pwc_*`` keys (the real cohort's ``pwc_real_*`` among them): the
        generated pathway frame against the scores of the generated expression frame, the sets from ``pathway_gene_matrix`` (genes x
        pathways 0/1, a DataFrame), the method ``consistency_method``; with the default nothing changes.
        ``enrichment=(real_cond, synth_cond)`` adds ``enrichment_fidelity``'s ``gsea_*`` keys on the expression frames; it needs
        ``pathway_gene_matrix`` (genes x pathways 0/1, a DataFrame), which is reindexed to the expression columns -- genes that are
        not among them drop out of their sets (``enrichment_names``: its ``names``; ``enrichment_permutations``: its
        ``permutations``); with the default None nothing changes.
        ``differential=(real_cond, synth_cond)`` adds ``differential_fidelity``'s ``de_*`` keys on the combined matrices (blocks
        ``mutations`` / ``expression`` / ``pathways``; ``differential_names``: its ``names``); with the default None nothing changes.
        ``marginals=True`` adds ``marginal_fidelity``'s ``marginal_*`` keys over every column of the combined matrices (blocks
        ``mutations`` / ``expression`` / ``pathways`` from the three frames' widths).
        ``survival=(real_train_surv, synth_surv, real_test, real_test_surv)`` adds ``survival_utility``'s ``survival_*`` keys, the
        cohorts as for ``utility=``: the combined real matrix trains, ``real_test`` is a (mutations, expression, pathways) triple
        of held-out real patients (or their combined matrix), each ``*_surv`` is [rows, 2] = (time, event).
        ``subtypes=K`` adds ``subtype_fidelity``'s ``subtype_*`` keys for K subtypes of the combined real matrix
        (``subtype_conditions=(real_cond, synth_cond)``: its ``conditions``).
        ``utility=(real_train_cond, synth_cond, real_test, real_test_cond)`` adds ``downstream_utility``'s ``utility_*`` keys: the
        combined real matrix is the training cohort, ``real_test`` a (mutations, expression, pathways) triple of held-out real
        patients (or their combined matrix); ``c2st=True`` adds ``discriminator_test``'s ``c2st_*`` keys on the combined matrices.
        ``correlation=True`` adds ``correlation_fidelity``'s ``corr_*`` keys (blocks ``mutations`` / ``expression`` / ``pathways``
        from the three frames' widths, strong pairs from |r_real| >= ``corr_strong``) and ``frechet=True`` its ``frechet_*`` keys, on the
        same combined matrices as the statistical tests.  ``prdc=True`` adds ``fidelity_diversity``'s keys (``prdc_k`` neighbours), on the same combined matrices as the statistical
        tests.  ``privacy=True`` adds ``privacy_audit``'s keys, on the same combined matrices as the statistical tests; ``holdout`` is
        then an optional (mutations, expression, pathways) triple of real patients the model never saw.  With a ``model`` (and
        ``membership`` = ((train data, train conditions), (holdout data, holdout conditions)), the rows as the model was trained
        on them) it also adds ``membership_audit``'s keys, each prefixed ``membership_``; without ``model`` nothing changes."""
        logger.info("=" * 50)
        logger.info("BIOLOGICAL VALIDATION")
        logger.info("=" * 50)
        all_results: Dict[str, float] = {}
        all_results.update(self.validate_mutation_cooccurrence(real_mutations, synth_mutations))
        if pathway_gene_matrix is not None:
            all_results.update(self.validate_pathway_coherence(real_expression, synth_expression, pathway_gene_matrix))
        all_results.update(self.validate_mutation_expression_correlation(synth_mutations, synth_expression, synth_pathways))
        parts_r = [real_mutations.values, real_expression.values, real_pathways.values]
        parts_s = [synth_mutations.values, synth_expression.values, synth_pathways.values]
        if all(isinstance(p, torch.Tensor) for p in parts_r + parts_s):          # DeviceFrame inputs: stay on the device
            real_combined, synth_combined = torch.cat(parts_r, dim=1), torch.cat(parts_s, dim=1)
        else:
            real_combined = np.concatenate([_host(p) for p in parts_r], axis=1)
            synth_combined = np.concatenate([_host(p) for p in parts_s], axis=1)
        all_results.update(self.statistical_tests(real_combined, synth_combined))
        if privacy:
            hold_combined = None
            if holdout is not None:
                parts_h = [p.values for p in holdout]
                if all(isinstance(p, torch.Tensor) for p in parts_h):
                    hold_combined = torch.cat(parts_h, dim=1)
                else:
                    hold_combined = np.concatenate([_host(p) for p in parts_h], axis=1)
            all_results.update(self.privacy_audit(real_combined, synth_combined, hold_combined))
            if model is not None:
                if membership is None:
                    raise ValueError("validate_all(model=...) needs membership=((train data, conditions), (holdout data, conditions))")
                all_results.update({f"membership_{k}": v for k, v in self.membership_audit(model, membership[0], membership[1]).items()})
        if prdc:
            all_results.update(self.fidelity_diversity(real_combined, synth_combined, k=prdc_k))
        if correlation or frechet:
            widths = {"mutations": parts_r[0].shape[1], "expression": parts_r[1].shape[1], "pathways": parts_r[2].shape[1]}
            second = self.correlation_fidelity(real_combined, synth_combined, blocks=widths, strong=corr_strong, frechet=frechet)
            all_results.update({key: v for key, v in second.items() if correlation or key.startswith("frechet_")})
        if utility is not None:
            if not isinstance(utility, (tuple, list)) or len(utility) != 4:
                raise ValueError("validate_all(utility=...) needs (real_train_cond, synth_cond, real_test, real_test_cond)")
            train_cond, synth_cond, test, test_cond = utility
            if isinstance(test, (tuple, list)):
                parts_t = [p.values for p in test]
                if all(isinstance(p, torch.Tensor) for p in parts_t):
                    test = torch.cat(parts_t, dim=1)
                else:
                    test = np.concatenate([_host(p) for p in parts_t], axis=1)
            all_results.update(self.downstream_utility(real_combined, train_cond, synth_combined, synth_cond, test, test_cond))
        if survival is not None:
            if not isinstance(survival, (tuple, list)) or len(survival) != 4:
                raise ValueError("validate_all(survival=...) needs (real_train_surv, synth_surv, real_test, real_test_surv)")
            train_surv, synth_surv, test, test_surv = survival
            if isinstance(test, (tuple, list)):
                parts_t = [p.values for p in test]
                if all(isinstance(p, torch.Tensor) for p in parts_t):
                    test = torch.cat(parts_t, dim=1)
                else:
                    test = np.concatenate([_host(p) for p in parts_t], axis=1)
            all_results.update(self.survival_utility(real_combined, train_surv, synth_combined, synth_surv, test, test_surv))
        if c2st:
            all_results.update(self.discriminator_test(real_combined, synth_combined))
        if subtypes is not None:
            all_results.update(self.subtype_fidelity(real_combined, synth_combined, int(subtypes), conditions=subtype_conditions))
        if marginals:
            widths = {"mutations": parts_r[0].shape[1], "expression": parts_r[1].shape[1], "pathways": parts_r[2].shape[1]}
            all_results.update(self.marginal_fidelity(real_combined, synth_combined, blocks=widths))
        if differential is not None:
            if not isinstance(differential, (tuple, list)) or len(differential) != 2:
                raise ValueError("validate_all(differential=...) needs (real_cond, synth_cond)")
            widths = {"mutations": parts_r[0].shape[1], "expression": parts_r[1].shape[1], "pathways": parts_r[2].shape[1]}
            all_results.update(self.differential_fidelity(real_combined, differential[0], synth_combined, differential[1],
                                                          names=differential_names, blocks=widths))
        if enrichment is not None:
            if not isinstance(enrichment, (tuple, list)) or len(enrichment) != 2:
                raise ValueError("validate_all(enrichment=...) needs (real_cond, synth_cond)")
            if pathway_gene_matrix is None or not hasattr(pathway_gene_matrix, "reindex"):
                raise ValueError("validate_all(enrichment=...) needs pathway_gene_matrix, a genes x pathways DataFrame")
            genes = [str(c) for c in real_expression.columns]
            if [str(c) for c in synth_expression.columns] != genes:
                raise ValueError("validate_all(enrichment=...) needs the same expression columns in both cohorts")
            membership_matrix = pathway_gene_matrix.reindex(list(real_expression.columns)).fillna(0)
            all_results.update(self.enrichment_fidelity(real_expression.values, enrichment[0], synth_expression.values, enrichment[1],
                                                        membership_matrix, names=enrichment_names,
                                                        permutations=int(enrichment_permutations)))
        if consistency:
            if pathway_gene_matrix is None or not hasattr(pathway_gene_matrix, "reindex"):
                raise ValueError("validate_all(consistency=True) needs pathway_gene_matrix, a genes x pathways DataFrame")
            all_results.update(self.pathway_consistency(synth_expression, synth_pathways, pathway_gene_matrix, real_expression,
                                                        real_pathways, method=consistency_method))
        if prognostic is not None:
            if not isinstance(prognostic, (tuple, list)) or len(prognostic) != 2:
                raise ValueError("validate_all(prognostic=...) needs (real_surv, synth_surv)")
            widths = {"mutations": parts_r[0].shape[1], "expression": parts_r[1].shape[1], "pathways": parts_r[2].shape[1]}
            all_results.update(self.prognostic_fidelity(real_combined, prognostic[0], synth_combined, prognostic[1], blocks=widths))
        if embedding:
            all_results.update(self.embedding_fidelity(real_combined, synth_combined, n_components=int(embedding_components)))
        logger.info("=" * 50)
        logger.info("VALIDATION SUMMARY")
        logger.info("=" * 50)
        for key, value in all_results.items():
            logger.info(f"{key}: {value}" if isinstance(value, str) else f"{key}: {value:.4f}")
        score = []
        if "mutation_frequency_correlation" in all_results:
            score.append(all_results["mutation_frequency_correlation"])
        if "cooccurrence_pattern_correlation" in all_results:
            score.append(all_results["cooccurrence_pattern_correlation"])
        if "mutual_exclusivity_violation_rate" in all_results:
            score.append(1 - all_results["mutual_exclusivity_violation_rate"])
        if "mutation_expression_violation_rate" in all_results:
            score.append(1 - all_results["mutation_expression_violation_rate"])
        if score:
            all_results["overall_biological_score"] = float(np.mean(score))
            logger.info(f"\nOverall Biological Score: {all_results['overall_biological_score']:.3f}")
        return all_results
