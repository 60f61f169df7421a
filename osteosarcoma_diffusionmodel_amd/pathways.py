"""Pathway feature engineering (the reference's utils/pathway_features.py, main.py step 3) and the pathway-consistency check
(DESIGN.md section 3.31): the third block of every patient vector, [mutation | expression | pathway], is a deterministic function
of the expression block -- per patient, the score of every gene set over that patient's genes.

  ``read_gmt`` / ``write_gmt``   gene sets in the GMT format; the package ships no list of its own, the user brings the file
  ``PathwayScorer``              name resolution (``min_genes``), the cohort fit (per-gene centre and scale for ``zscore``, the
                                 per-pathway mean and sd ``prepare_data`` standardises with) and ``score``: one
                                 ``DeviceKernels.pathway_scores`` call (``osd_val_pathway_scores``) per matrix
  ``compute_pathway_features``   step 3: the two aligned CSVs in, ``pathway_scores.csv``, ``pathway_mutation_scores.csv`` and
                                 ``gene_pathway_matrix.csv`` out
  ``pathway_consistency``        does a generated patient's pathway block agree with the scores of that same patient's generated
                                 expression?  The six column sums of ``DeviceKernels.pathway_agreement`` and float64 host code

Methods: ``mean`` (the reference's: the mean of the set's genes), ``zscore`` (the combined z-score of Lee et al. 2008) and ``ssgsea``
(Barbie et al. 2009: the integral of the weighted running sum over the patient's ranked genes, in its closed form over mid-ranks,
which GSVA's ``ssgsea`` without its final normalisation also computes).  The kernels object is an argument, so the CPU tests drive
the same code over a NumPy stand-in."""
from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import enrichment as EN

logger = logging.getLogger(__name__)

METHODS = ("mean", "zscore", "ssgsea")          # the method numbers of osd_val_pathway_scores
MAX_SET = 1024                                  # members of a set osd_val_pathway_scores takes


# ---- gene sets --------------------------------------------------------------------------------------------------------------------
def read_gmt(path) -> Dict[str, List[str]]:
    """An ordered ``{name: [gene symbols]}`` from a GMT file: one set per line, tab-separated -- name, description (ignored, may be
    blank), members.  Blank lines are skipped, empty members dropped, a member listed twice is kept once (its first place); a name
    that occurs twice is a ValueError."""
    sets: Dict[str, List[str]] = {}
    with open(path, "r", encoding="utf-8") as fh:
        for n, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            cells = line.split("\t")
            name = cells[0].strip()
            if not name or len(cells) < 2:
                raise ValueError(f"{path}:{n}: a GMT line holds a name, a description and the members, tab-separated")
            if name in sets:
                raise ValueError(f"{path}:{n}: the set {name!r} occurs twice")
            sets[name] = list(dict.fromkeys(c.strip() for c in cells[2:] if c.strip()))
    return sets


def write_gmt(sets, path, descriptions: Optional[Dict[str, str]] = None) -> None:
    """``sets`` (an ordered ``{name: gene symbols}``) as a GMT file; the description column is blank unless given."""
    with open(path, "w", encoding="utf-8") as fh:
        for name, members in sets.items():
            cells = [str(name), str((descriptions or {}).get(name, ""))] + [str(g) for g in members]
            if any("\t" in c or "\n" in c for c in cells):
                raise ValueError(f"the set {name!r} holds a tab or a line break")
            fh.write("\t".join(cells) + "\n")


def gene_pathway_matrix(gene_sets):
    """The reference's ``create_gene_pathway_matrix``: a 0/1 DataFrame, one row per gene symbol of any set (sorted), one column per
    set (input order) -- every set, also those a cohort is too narrow for."""
    import pandas as pd
    genes = sorted({str(g) for members in gene_sets.values() for g in members})
    row = {g: i for i, g in enumerate(genes)}
    m = np.zeros((len(genes), len(gene_sets)), dtype=np.int64)
    for s, members in enumerate(gene_sets.values()):
        m[[row[str(g)] for g in members], s] = 1
    return pd.DataFrame(m, index=genes, columns=[str(n) for n in gene_sets])


def rank_table(D: int, alpha: float = 0.25) -> np.ndarray:
    """float64 [2 D + 1]: T[k] = (k / 2) ** alpha, the weight of the mid-rank k / 2 (``alpha`` = 0: all ones)."""
    return np.power(np.arange(2 * int(D) + 1, dtype=np.float64) / 2.0, float(alpha))


def resolve_sets(gene_sets, genes: Sequence, min_genes: int = 5) -> Tuple[List[str], List[np.ndarray], List[str]]:
    """(names, sets, skipped names) over the columns ``genes``.  ``gene_sets``: an ordered name -> gene symbols mapping (a symbol
    that is no column drops out, one listed twice counts once; the members keep the order of the listing), a name -> column indices
    mapping or a genes x sets 0/1 DataFrame (``enrichment.select_sets``: members sorted).  A set with fewer than ``min_genes`` genes
    present -- the reference's ``len(common_genes) < 5`` -- or more than min(1024, D - 1) is skipped.  ``names`` keeps the input
    order."""
    D = len(genes)
    if int(min_genes) < 1:
        raise ValueError("min_genes must be at least 1")
    if hasattr(gene_sets, "columns"):
        all_names = [str(c) for c in gene_sets.columns]
        names, sets, _ = EN.select_sets(gene_sets, D, int(min_genes), MAX_SET, columns=list(genes))
        return names, sets, [n for n in all_names if n not in set(names)]
    if not hasattr(gene_sets, "items"):
        raise ValueError("gene_sets must be a name -> members mapping or a genes x sets 0/1 DataFrame")
    by_symbol = any(isinstance(g, str) for members in gene_sets.values() for g in members)
    if not by_symbol:
        all_names = [str(n) for n in gene_sets]
        names, sets, _ = EN.select_sets(gene_sets, D, int(min_genes), MAX_SET)
        return names, sets, [n for n in all_names if n not in set(names)]
    col = {}
    for i, g in enumerate(genes):
        col.setdefault(str(g), i)
    names, sets, skipped = [], [], []
    hi = min(MAX_SET, D - 1)
    for name, members in gene_sets.items():
        idx = list(dict.fromkeys(col[str(g)] for g in members if str(g) in col))
        if len(idx) < int(min_genes) or len(idx) > hi:
            skipped.append(str(name))
            continue
        names.append(str(name))
        sets.append(np.asarray(idx, dtype=np.int64))
    if len(set(names)) != len(names):
        raise ValueError("the gene sets need distinct names")
    return names, sets, skipped


def _device_kernels(device: torch.device):
    """The kernels a scorer uses when none are given: ``validation.DeviceKernels`` -- there is no CPU fallback."""
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("the pathway kernels run on a ROCm device; there is no CPU fallback")
    from .validation import DeviceKernels
    return DeviceKernels(device)


def _is_frame(a) -> bool:
    return hasattr(a, "columns") and hasattr(a, "values")


def _on_device(a, device) -> torch.Tensor:
    """The fp32 matrix of a frame, a tensor or an array on ``device``.  A tensor that already lives there with contiguous rows -- a
    column slice of the combined [mutation | expression | pathway] matrix -- is passed on as it is, row stride and all: the kernels
    read it in place.  Anything else is converted and copied."""
    from .validation import _dev, _rows_view
    t = a.values if _is_frame(a) else a
    dev = torch.device(device)
    there = isinstance(t, torch.Tensor) and t.device.type == dev.type and (dev.index is None or t.device.index == dev.index)
    if there and t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] >= 1:
        return _rows_view(t)
    return _dev(a, device)


# ---- the scorer -------------------------------------------------------------------------------------------------------------------
class PathwayScorer:
    """Per-patient scores of the gene sets ``gene_sets`` (``resolve_sets``) over the expression columns ``genes``.  ``method``:
    ``mean``, ``zscore`` or ``ssgsea`` (``alpha``: the exponent of the rank weights); ``.names`` the kept sets in input order,
    ``.sets`` their column indices, ``.skipped`` the number of sets dropped (``.skipped_names``).  ``kernels``: the object whose
    ``pathway_scores`` and ``col_centered_moments`` run (default: ``validation.DeviceKernels`` on ``device``)."""

    def __init__(self, gene_sets, genes, method: str = "mean", alpha: float = 0.25, min_genes: int = 5, device="cuda", kernels=None):
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, got {method!r}")
        if not 0.0 <= float(alpha) <= 16.0:
            raise ValueError("alpha must lie in [0, 16]")
        self.genes = [g if isinstance(g, str) else (int(g) if isinstance(g, (int, np.integer)) else str(g)) for g in genes]
        self.method, self.alpha, self.min_genes = method, float(alpha), int(min_genes)
        if len(self.genes) < 2 or len(self.genes) > 32768:
            raise ValueError("between 2 and 32768 expression columns are needed")
        self.names, self.sets, self.skipped_names = resolve_sets(gene_sets, self.genes, self.min_genes)
        if not self.names:
            raise ValueError(f"no gene set has {self.min_genes} genes among the columns")
        self.skipped = len(self.skipped_names)
        self.k = kernels if kernels is not None else _device_kernels(torch.device(device))
        self.device = torch.device(getattr(self.k, "device", device))            # the tensors live where the kernels run
        self.center = self.scale = self.mu = self.sd = None
        self._table = rank_table(len(self.genes), self.alpha) if method == "ssgsea" else None

    # -- inputs ---------------------------------------------------------------------------------------------------------------------
    def _matrix(self, expression) -> torch.Tensor:
        """The fp32 [rows, D] tensor on the scorer's device; a frame's columns are put into the order of ``genes`` by name."""
        if _is_frame(expression):
            cols = [c if isinstance(c, str) else (int(c) if isinstance(c, (int, np.integer)) else str(c)) for c in expression.columns]
            if cols != self.genes:
                missing = [g for g in self.genes if g not in set(cols)]
                if missing:
                    raise ValueError(f"the expression frame lacks {len(missing)} of the scorer's genes, e.g. {missing[:3]}")
                expression = expression[self.genes]
        x = _on_device(expression, self.device)
        if x.dim() != 2 or x.shape[1] != len(self.genes) or x.shape[0] < 1:
            raise ValueError(f"the expression matrix must be [rows >= 1, {len(self.genes)}], got {tuple(x.shape)}")
        return x

    def raw_scores(self, x: torch.Tensor) -> torch.Tensor:
        """float64 [rows, S] on the device from the fp32 device tensor x [rows, D]."""
        if self.method == "zscore" and self.center is None:
            raise ValueError("zscore needs the per-gene centre and scale: call fit(expression) first")
        return self.k.pathway_scores(x, self.sets, self.method, center=self.center, scale=self.scale, rank_table=self._table)

    # -- fit ------------------------------------------------------------------------------------------------------------------------
    def fit(self, expression) -> "PathwayScorer":
        """Stores, from the cohort ``expression``: for ``zscore`` the per-gene centre (the mean) and scale (1 / sd, ddof = 1; 0 where
        the sd is 0), both rounded to fp32 as the kernel reads them (two ``col_centered_moments`` passes: the second is centred at
        the first's mean); and the mean and sd (ddof = 1) of every pathway's scores over the cohort, what ``prepare_data`` standardises
        ``pathway_scores.csv`` with."""
        x = self._matrix(expression)
        n = int(x.shape[0])
        if n < 2:
            raise ValueError("a fit needs two patients at least")
        if self.method == "zscore":
            s, _ = self.k.col_centered_moments(x)
            c = (np.asarray(s, dtype=np.float64) / n).astype(np.float32)
            s, q = self.k.col_centered_moments(x, c)
            s, q = np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
            var = np.maximum(q - s * s / n, 0.0) / (n - 1)
            with np.errstate(divide="ignore"):
                self.scale = np.where(var > 0, 1.0 / np.sqrt(var), 0.0).astype(np.float32)
            self.center = c
        p = self.raw_scores(x).detach().cpu().numpy()
        self.mu, self.sd = p.mean(axis=0), p.std(axis=0, ddof=1)
        return self

    @property
    def isd(self) -> np.ndarray:
        """1 / (sd + 1e-8): ``prepare_data`` divides by std + 1e-8."""
        if self.mu is None:
            raise ValueError("the scorer is not fitted: call fit(expression) first")
        return 1.0 / (self.sd + 1e-8)

    # -- score ----------------------------------------------------------------------------------------------------------------------
    def score(self, expression, standardize: bool = False):
        """The scores of every row: a DataFrame (index kept, columns ``names``) for a DataFrame, a ``DeviceFrame`` for a
        ``DeviceFrame`` and a float64 device tensor [rows, S] for a tensor or an array.  ``standardize=True``: (p - mean) / (sd +
        1e-8) with the fitted cohort's figures."""
        from .validation import DeviceFrame
        p = self.raw_scores(self._matrix(expression))
        if standardize:
            isd = self.isd
            p = (p - torch.from_numpy(self.mu).to(p.device)) * torch.from_numpy(isd).to(p.device)
        if isinstance(expression, DeviceFrame):
            return DeviceFrame(p, self.names)
        if _is_frame(expression):
            import pandas as pd
            return pd.DataFrame(p.detach().cpu().numpy(), index=expression.index, columns=self.names)
        return p

    # -- checkpoint -----------------------------------------------------------------------------------------------------------------
    def state(self) -> Dict[str, np.ndarray]:
        """A dict of numpy arrays (strings as unicode arrays, absent fits as empty arrays) that ``from_state`` turns back into an
        equal scorer."""
        offsets = np.zeros(len(self.sets) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(m) for m in self.sets])
        none = np.zeros(0)
        return {"genes": np.array([str(g) for g in self.genes]), "genes_are_indices": np.array(all(isinstance(g, int) for g in self.genes)),
                "names": np.array(self.names), "skipped_names": np.array(self.skipped_names, dtype=str),
                "set_offsets": offsets, "set_members": np.concatenate(self.sets).astype(np.int64),
                "method": np.array(self.method), "alpha": np.array(self.alpha), "min_genes": np.array(self.min_genes),
                "center": none.astype(np.float32) if self.center is None else self.center.copy(),
                "scale": none.astype(np.float32) if self.scale is None else self.scale.copy(),
                "mu": none if self.mu is None else self.mu.copy(), "sd": none if self.sd is None else self.sd.copy()}

    @classmethod
    def from_state(cls, state, device="cuda", kernels=None) -> "PathwayScorer":
        genes = [str(g) for g in np.asarray(state["genes"]).tolist()]
        if bool(np.asarray(state["genes_are_indices"])):
            genes = [int(g) for g in genes]
        off, mem = np.asarray(state["set_offsets"], dtype=np.int64), np.asarray(state["set_members"], dtype=np.int64)
        names = [str(n) for n in np.asarray(state["names"]).tolist()]
        sets = {n: mem[off[i]:off[i + 1]] for i, n in enumerate(names)}
        self = cls.__new__(cls)
        self.genes, self.method = genes, str(np.asarray(state["method"]))
        self.alpha, self.min_genes = float(np.asarray(state["alpha"])), int(np.asarray(state["min_genes"]))
        if self.method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, got {self.method!r}")
        self.names, self.sets = names, [np.asarray(m, dtype=np.int64) for m in sets.values()]
        D = len(genes)
        if any(m.size < 1 or m.size > min(MAX_SET, D - 1) or m.min() < 0 or m.max() >= D or np.unique(m).size != m.size for m in self.sets):
            raise ValueError("the state's sets do not fit its genes")
        self.skipped_names = [str(n) for n in np.asarray(state["skipped_names"]).tolist()]
        self.skipped = len(self.skipped_names)
        self.k = kernels if kernels is not None else _device_kernels(torch.device(device))
        self.device = torch.device(getattr(self.k, "device", device))
        opt = lambda key, dt: None if np.asarray(state[key]).size == 0 else np.asarray(state[key], dtype=dt).copy()
        self.center, self.scale, self.mu, self.sd = opt("center", np.float32), opt("scale", np.float32), opt("mu", np.float64), opt("sd", np.float64)
        self._table = rank_table(D, self.alpha) if self.method == "ssgsea" else None
        return self


# ---- main.py step 3 ---------------------------------------------------------------------------------------------------------------
def compute_pathway_features(config: dict, device="cuda", kernels=None):
    """The reference's step 3 from ``config["data"]``: reads ``expression_matrix_aligned.csv`` and ``mutation_matrix_aligned.csv``
    under ``processed_dir``, takes the gene sets from ``gene_sets_file`` (GMT) and the method from ``pathway_scoring`` (default
    ``mean``; ``pathway_alpha``: the ``ssgsea`` exponent, default 0.25), and writes beside them ``pathway_scores.csv`` (the
    expression scores, unstandardised: ``prepare_data`` standardises what it reads), ``pathway_mutation_scores.csv`` (the share of
    every set's genes that are mutated; the sets with ``min_genes`` genes among the mutation columns, none: no columns) and
    ``gene_pathway_matrix.csv`` (``gene_pathway_matrix``).  Every file is written under a temporary name and renamed into place,
    ``pathway_scores.csv`` last.  Returns the three frames."""
    import pandas as pd
    data = config["data"]
    if not data.get("gene_sets_file"):
        raise ValueError("config['data']['gene_sets_file'] names the GMT file the pathway scores are computed from")
    processed = Path(data["processed_dir"])
    method = data.get("pathway_scoring", "mean")
    gene_sets = read_gmt(data["gene_sets_file"])
    expression = pd.read_csv(processed / "expression_matrix_aligned.csv", index_col=0)
    mutations = pd.read_csv(processed / "mutation_matrix_aligned.csv", index_col=0)
    scorer = PathwayScorer(gene_sets, list(expression.columns), method=method, alpha=float(data.get("pathway_alpha", 0.25)),
                           device=device, kernels=kernels)
    if method == "zscore":
        scorer.fit(expression)
    scores = scorer.score(expression)
    logger.info(f"Computed {scores.shape[1]} pathway scores ({method}); {scorer.skipped} sets skipped")
    if resolve_sets(gene_sets, list(mutations.columns), scorer.min_genes)[0]:
        burden = PathwayScorer(gene_sets, list(mutations.columns), method="mean", device=device, kernels=scorer.k).score(mutations)
    else:                                            # no set has enough genes among the mutation columns: the reference's empty frame
        burden = pd.DataFrame(index=mutations.index)
    matrix = gene_pathway_matrix(gene_sets)
    for frame, name in ((burden, "pathway_mutation_scores.csv"), (matrix, "gene_pathway_matrix.csv"), (scores, "pathway_scores.csv")):
        part = processed / f".{name}.{os.getpid()}.part"     # a reader never sees a half-written file: written aside, then renamed
        frame.to_csv(part)
        os.replace(part, processed / name)
    return scores, burden, matrix


# ---- the consistency check --------------------------------------------------------------------------------------------------------
def agreement_rows(sums, used) -> Dict[str, np.ndarray]:
    """Per pathway, from the sums of ``DeviceKernels.pathway_agreement`` ([S, 6]) and the rows used ([S]): ``pearson`` r(g, z),
    ``rmse`` sqrt(mean (g - z)^2), ``bias`` mean g - mean z, ``sd_ratio`` sd g / sd z, plus ``var_z`` and ``sq_err`` (the centred sum
    of squares of z and sum (g - z)^2: the pooled R^2's terms) and ``n``.  NaN where no row is left; ``pearson`` and ``sd_ratio`` are
    NaN where z or g is constant."""
    sums, n = np.asarray(sums, dtype=np.float64), np.asarray(used, dtype=np.float64)
    sz, sg, szz, sgg, szg, sdd = (sums[:, i] for i in range(6))
    with np.errstate(divide="ignore", invalid="ignore"):
        mz, mg = sz / n, sg / n
        vz, vg = np.maximum(szz - n * mz * mz, 0.0), np.maximum(sgg - n * mg * mg, 0.0)
        cov = szg - n * mz * mg
        live = (vz > 1e-12 * np.maximum(szz, 1e-300)) & (vg > 1e-12 * np.maximum(sgg, 1e-300))
        r = np.where(live, cov / np.sqrt(vz * vg), np.nan)
        ratio = np.where(live, np.sqrt(vg / vz), np.nan)
        rmse = np.sqrt(sdd / n)
    return {"pearson": np.clip(r, -1.0, 1.0), "rmse": rmse, "bias": mg - mz, "sd_ratio": ratio, "var_z": np.where(n > 0, vz, np.nan),
            "sq_err": np.where(n > 0, sdd, np.nan), "n": np.asarray(used, dtype=np.int64)}


def agreement_summary(rows: Dict[str, np.ndarray], names: Sequence[str], total_rows: int, skipped: int, prefix: str = "pwc_") -> Dict[str, float]:
    """The ``pwc_*`` keys from ``agreement_rows`` (NaNs left out of the means and extremes; NaN and '' where nothing is left)."""
    def over(v, fn):
        v = v[~np.isnan(v)]
        return float(fn(v)) if v.size else float("nan")

    def where(v, fn):
        return str(names[int(fn(np.where(np.isnan(v), -np.inf if fn is np.argmax else np.inf, v)))]) if (~np.isnan(v)).any() else ""

    r, rmse = rows["pearson"], rows["rmse"]
    ok = ~np.isnan(rows["var_z"]) & ~np.isnan(rows["sq_err"])
    den = float(rows["var_z"][ok].sum())
    return {
        f"{prefix}pearson_mean": over(r, np.mean), f"{prefix}pearson_min": over(r, np.min), f"{prefix}pearson_min_pathway": where(r, np.argmin),
        f"{prefix}rmse_mean": over(rmse, np.mean), f"{prefix}rmse_max": over(rmse, np.max), f"{prefix}rmse_max_pathway": where(rmse, np.argmax),
        f"{prefix}abs_bias_mean": over(np.abs(rows["bias"]), np.mean), f"{prefix}sd_ratio_mean": over(rows["sd_ratio"], np.mean),
        f"{prefix}r2": 1.0 - float(rows["sq_err"][ok].sum()) / den if den > 0 else float("nan"),
        f"{prefix}pathways": len(names), f"{prefix}pathways_skipped": int(skipped),
        f"{prefix}constant": int(np.isnan(r).sum()), f"{prefix}rows_nonfinite": int((int(total_rows) - rows["n"]).sum()),
    }


def _block(pathways, names: Sequence[str], device, rows: int) -> torch.Tensor:
    """The fp32 [rows, S] device tensor of a pathway block: a frame's columns are matched to ``names`` by name, a bare matrix must hold
    exactly the kept sets, in their order."""
    if _is_frame(pathways):
        have = {str(c) for c in pathways.columns}
        missing = [n for n in names if n not in have]
        if missing:
            raise ValueError(f"the pathway block lacks {len(missing)} of the kept sets, e.g. {missing[:3]}")
        if [str(c) for c in pathways.columns] != list(names):
            pathways = pathways[list(names)]
    g = _on_device(pathways, device)
    if g.dim() != 2 or g.shape[1] != len(names):
        what = "narrower" if g.dim() == 2 and g.shape[1] < len(names) else "wider"
        raise ValueError(f"the pathway block is {what} than the {len(names)} kept sets: name its columns, or pass exactly these sets")
    if g.shape[0] != rows:
        raise ValueError(f"the pathway block holds {g.shape[0]} rows, the expression matrix {rows}")
    return g


def pathway_consistency(comm, k, device, synth_expression, synth_pathways, gene_sets, real_expression, real_pathways=None,
                        method: str = "mean", alpha: float = 0.25, min_genes: int = 5):
    """(summary, rows) of ``BiologicalValidator.pathway_consistency``: ``comm`` sums the synthetic shards' accumulators
    (``parallel.ShardComm``), ``k`` holds the kernels, ``device`` the tensors."""
    if _is_frame(real_expression):
        genes = list(real_expression.columns)
    else:
        shape = tuple(real_expression.shape)
        if len(shape) != 2:
            raise ValueError("real_expression must be a [patients, genes] matrix")
        genes = list(range(shape[1]))
    scorer = PathwayScorer(gene_sets, genes, method=method, alpha=alpha, min_genes=min_genes, device=device, kernels=k)
    width = lambda a: int(a.shape[1]) if len(tuple(a.shape)) == 2 else -1
    if width(synth_expression) != len(genes):
        raise ValueError(f"the synthetic expression matrix must have the real one's {len(genes)} genes, got {width(synth_expression)}")
    x_real = scorer._matrix(real_expression)
    scorer.fit(x_real)
    mu, isd = scorer.mu, scorer.isd
    x = scorer._matrix(synth_expression)
    g = _block(synth_pathways, scorer.names, scorer.device, int(x.shape[0]))
    local = k.pathway_agreement(scorer.raw_scores(x), g, mu, isd)
    sums, used = comm.sum(local["sums"]), comm.sum(local["used"])
    total = int(comm.sum(np.array([x.shape[0]], dtype=np.int64))[0])
    rows = {"synthetic": agreement_rows(sums, used), "names": list(scorer.names), "skipped": list(scorer.skipped_names),
            "mu": mu, "sd": scorer.sd}
    summary = agreement_summary(rows["synthetic"], scorer.names, total, scorer.skipped)
    if real_pathways is not None:
        gr = _block(real_pathways, scorer.names, scorer.device, int(x_real.shape[0]))
        own = k.pathway_agreement(scorer.raw_scores(x_real), gr, mu, isd)
        rows["real"] = agreement_rows(own["sums"], own["used"])
        summary.update(agreement_summary(rows["real"], scorer.names, int(x_real.shape[0]), scorer.skipped, prefix="pwc_real_"))
    return summary, rows
