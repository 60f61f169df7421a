"""Float64 restatement of the feature transforms (the rule is the comment block of ``osd_xf_apply`` in
include/osdiff.h) and the case generators of test_transform_cpu.py / test_gpu_transform.py.  Written from the rule with explicit
``searchsorted`` left and right -- ``np.interp`` does something else on tied knots -- and without a product import."""
import functools

import numpy as np
import torch

IDENTITY, STANDARD, QUANTILE = 0, 1, 2
EPS = 2.0 ** -23
STRIP = 32                      # columns of a workgroup (csrc/transform.hip: XF_STRIP)


# ---- fit ----------------------------------------------------------------------------------------------------------------------------
def ref_levels(Q):
    """float32 [Q]: Phi^-1(clip(i / (Q - 1), 1e-7, 1 - 1e-7)), antisymmetrised in float64, rounded once.  Phi^-1 is torch's float64
    ``ndtri``: another implementation than the product's."""
    p = np.clip(np.arange(Q, dtype=np.float64) / (Q - 1), 1e-7, 1.0 - 1e-7)
    z = torch.special.ndtri(torch.from_numpy(p)).numpy()
    return (0.5 * (z - z[::-1])).astype(np.float32)


def ref_knots(col, Q):
    """float32 [Q]: the quantiles of the finite entries of ``col`` at levels i / (Q - 1), linear between order statistics, the position
    i (n - 1) / (Q - 1) split into quotient and remainder in integers."""
    s = np.sort(np.asarray(col, dtype=np.float64)[np.isfinite(col)])
    n = s.shape[0]
    out = np.empty(Q, dtype=np.float64)
    for i in range(Q):
        q, r = divmod(i * (n - 1), Q - 1)
        out[i] = s[q] + (s[min(q + 1, n - 1)] - s[q]) * (r / (Q - 1))
    return out.astype(np.float32)


# ---- maps ---------------------------------------------------------------------------------------------------------------------------
def ref_forward(x, kind, knots, levels, center, scale):
    """(ref float64 [rows, D], exact bool [rows, D], tol float64 [rows, D]) for the fp32 inputs ``x`` and the fp32 tables.  Where
    ``exact``, the rule returns a table entry, a mid-rank mean (formed in fp32, as the rule states it), a copy or NaN and ``ref`` holds
    that fp32 value: bit equality is demanded.  Elsewhere |device - ref| <= tol: 8 x 2^-23 x the larger bracketing level for an
    interpolated value (five fp32 roundings at most), and for a standard column two roundings of (x - c) / s."""
    rows, D = x.shape
    Q = levels.shape[0]
    ref = np.empty((rows, D), dtype=np.float64)
    exact = np.ones((rows, D), dtype=bool)
    tol = np.zeros((rows, D), dtype=np.float64)
    zl, zl64 = levels, levels.astype(np.float64)
    half = np.float32(0.5)
    for f in range(D):
        xf = x[:, f]
        if kind[f] == IDENTITY:
            ref[:, f] = xf
        elif kind[f] == STANDARD:
            c, s = np.float64(center[f]), np.float64(scale[f])
            with np.errstate(invalid="ignore"):
                ref[:, f] = (xf.astype(np.float64) - c) / s
                fin = np.isfinite(xf)
                exact[:, f] = ~fin                                   # NaN -> NaN, +-inf -> +-inf
                tol[:, f] = np.where(fin, 2 * EPS * (np.abs(xf.astype(np.float64)) + abs(c)) / abs(s), 0.0)
        else:
            k, k64 = knots[f], knots[f].astype(np.float64)
            nan = np.isnan(xf)
            xs = np.where(nan, np.float32(0), xf)
            lb, ub = np.searchsorted(k, xs, side="left"), np.searchsorted(k, xs, side="right")
            out = np.empty(rows, dtype=np.float64)
            for r in range(rows):
                if nan[r]:
                    out[r] = np.nan
                elif ub[r] == 0:
                    out[r] = zl[0]
                elif lb[r] == Q:
                    out[r] = zl[Q - 1]
                elif ub[r] > lb[r]:
                    out[r] = half * (zl[(lb[r] + ub[r] - 1) >> 1] + zl[(lb[r] + ub[r]) >> 1])      # fp32 arithmetic
                else:
                    j = lb[r] - 1
                    t = (np.float64(xs[r]) - k64[j]) / (k64[j + 1] - k64[j])
                    out[r] = zl64[j] + t * (zl64[j + 1] - zl64[j])
                    exact[r, f] = False
                    tol[r, f] = 8 * EPS * max(abs(zl64[j]), abs(zl64[j + 1]))
            ref[:, f] = out
    return ref, exact, tol


def ref_inverse(z, kind, knots, levels, center, scale):
    """As ``ref_forward`` for the inverse maps.  Exact: the clamps, a z that is a level (t = 0), a z inside a plateau's interval (the
    bracketing knots are equal), identity columns, NaN.  Interpolated: 8 x 2^-23 x the larger bracketing knot."""
    rows, D = z.shape
    Q = levels.shape[0]
    ref = np.empty((rows, D), dtype=np.float64)
    exact = np.ones((rows, D), dtype=bool)
    tol = np.zeros((rows, D), dtype=np.float64)
    zl, zl64 = levels, levels.astype(np.float64)
    for f in range(D):
        zf = z[:, f]
        if kind[f] == IDENTITY:
            ref[:, f] = zf
        elif kind[f] == STANDARD:
            c, s = np.float64(center[f]), np.float64(scale[f])
            with np.errstate(invalid="ignore"):
                ref[:, f] = zf.astype(np.float64) * s + c
                fin = np.isfinite(zf)
                exact[:, f] = ~fin
                tol[:, f] = np.where(fin, 2 * EPS * (np.abs(zf.astype(np.float64) * s) + abs(c)), 0.0)
        else:
            k, k64 = knots[f], knots[f].astype(np.float64)
            nan = np.isnan(zf)
            zs = np.where(nan, np.float32(0), zf)
            ub = np.searchsorted(zl, zs, side="right")
            out = np.empty(rows, dtype=np.float64)
            for r in range(rows):
                if nan[r]:
                    out[r] = np.nan
                elif zs[r] <= zl[0]:
                    out[r] = k[0]
                elif zs[r] >= zl[Q - 1]:
                    out[r] = k[Q - 1]
                else:
                    j = ub[r] - 1                                    # zl[j] <= z < zl[j + 1]
                    if k[j] == k[j + 1] or zs[r] == zl[j]:
                        out[r] = k[j]
                    else:
                        t = (np.float64(zs[r]) - zl64[j]) / (zl64[j + 1] - zl64[j])
                        out[r] = k64[j] + t * (k64[j + 1] - k64[j])
                        exact[r, f] = False
                        tol[r, f] = 8 * EPS * max(abs(k64[j]), abs(k64[j + 1]))
            ref[:, f] = out
    return ref, exact, tol


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_matches(dev, ref, exact, tol, what):
    """The device's fp32 result against ``ref_forward`` / ``ref_inverse``: bit equality where exact (NaN matches NaN), else within tol.
    Returns the largest |device - ref| / tol over the interpolated entries (0 without one)."""
    dev = np.asarray(dev)
    assert dev.dtype == np.float32 and dev.shape == ref.shape, what
    want = ref.astype(np.float32)
    nan = np.isnan(want)
    assert (np.isnan(dev) == nan).all(), f"{what}: NaN pattern differs"
    eq = (bits(dev) == bits(want)) | nan
    bad = exact & ~eq
    assert not bad.any(), (f"{what}: {int(bad.sum())} exact entries differ in bits, first at {tuple(np.argwhere(bad)[0])}: "
                           f"device {dev[bad][0]!r}, rule {want[bad][0]!r}")
    loose = ~exact
    if not loose.any():
        return 0.0
    err = np.abs(dev.astype(np.float64)[loose] - ref[loose])
    worst = float((err / tol[loose]).max())
    over = err > tol[loose]
    assert not over.any(), f"{what}: {int(over.sum())} interpolated entries beyond the bound; worst error / bound = {worst:.3f}"
    return worst


# ---- cases --------------------------------------------------------------------------------------------------------------------------
SEGMENTS = (5, 27, 8, 24, 32, 3, 29, 64)        # kind changes at columns 5, 32, 40, 64, 96, 99, 128, 192 (+ 192 n): inside and on strip boundaries


def mixed_kinds(D):
    """int32 [D]: quantile, identity, standard, quantile, ... over SEGMENTS, so that the kind changes inside strips (5, 40, 99) and on
    their boundaries (32, 64, 96, 128, 192)."""
    kind = np.empty(D, dtype=np.int32)
    f, i = 0, 0
    order = (QUANTILE, IDENTITY, STANDARD)
    while f < D:
        w = SEGMENTS[i % len(SEGMENTS)]
        kind[f:f + w] = order[i % 3]
        f, i = f + w, i + 1
    return kind


def _column_knots(rs, Q, style):
    """float32 [Q], non-decreasing: one quantile column's knots in one of six styles."""
    if style == 0:                                                  # continuous, positive
        v = rs.normal(5.0, 3.0, Q)
    elif style == 1:                                                # a constant column
        v = np.full(Q, 2.5)
    elif style == 2:                                                # subnormal gaps between normal numbers: 2^-120 + i 2^-140
        v = 2.0 ** -120 + np.arange(Q) * 2.0 ** -140
    elif style == 3:                                                # zero-inflated: 30 % zeros, then a log-normal tail
        nz = max(1, int(round(0.3 * Q)))
        v = np.concatenate([np.zeros(nz), np.exp(rs.normal(1.0, 1.0, Q - nz))])
    elif style == 4:                                                # steps of 0.5, both signs: many plateaus
        v = np.round(rs.normal(0.0, 2.0, Q) * 2) / 2
    else:                                                           # both signs, five decades
        v = rs.normal(0.0, 1.0, Q) * 10.0 ** rs.uniform(-2, 3, Q)
    return np.sort(v.astype(np.float32)) + np.float32(0.0)         # no -0.0 among the knots: k + t * 0 is +0.0, equal but other bits


@functools.lru_cache(maxsize=None)
def make_case(rows, D, Q, seed=0, all_quantile=False):
    """One read-only case: tables (``kind`` mixed over SEGMENTS, ``knots`` in the six styles of ``_column_knots`` cycling over the
    quantile columns, ``levels``, ``center``, ``scale``) and the inputs ``x`` (forward) and ``z`` (inverse), fp32 [rows, D].  Element
    (r, f) takes input class (r + f) % 10: a knot; the midpoint of two neighbouring knots; a random point between two knots; below
    k[0]; above k[Q-1]; +inf; -inf; NaN; k[0] or k[Q-1] itself; anywhere in the range -- and likewise for z over the levels."""
    rs = np.random.default_rng(1000003 * seed + 7919 * rows + 31 * D + Q)
    kind = np.full(D, QUANTILE, dtype=np.int32) if all_quantile else mixed_kinds(D)
    levels = ref_levels(Q)
    knots = np.zeros((D, Q), dtype=np.float32)
    qcols = np.flatnonzero(kind == QUANTILE)
    for n, f in enumerate(qcols):
        knots[f] = _column_knots(rs, Q, n % 6)
    center = np.where(kind == STANDARD, rs.normal(0, 2, D), 0.0).astype(np.float32)
    scale = np.where(kind == STANDARD, rs.uniform(0.1, 3, D), 1.0).astype(np.float32)

    def inputs(table_of):
        out = rs.normal(0, 3, (rows, D)).astype(np.float32)           # identity and standard columns keep these
        r_idx, f_idx = np.meshgrid(np.arange(rows), np.arange(D), indexing="ij")
        cls = (r_idx + f_idx) % 10
        out[cls == 5], out[cls == 6], out[cls == 7] = np.inf, -np.inf, np.nan
        for f in qcols:
            tab = table_of(f)
            j = rs.integers(0, Q - 1, rows)
            u = rs.random(rows).astype(np.float32)
            lo, hi = tab[j], tab[j + 1]
            span = max(float(tab[-1]) - float(tab[0]), abs(float(tab[0])), 1e-30)
            col = out[:, f]
            c = cls[:, f]
            col[c == 0] = lo[c == 0]
            col[c == 1] = (np.float32(0.5) * (lo + hi))[c == 1]
            col[c == 2] = (lo + u * (hi - lo))[c == 2]
            col[c == 3] = np.float32(float(tab[0]) - 0.37 * span)
            col[c == 4] = np.float32(float(tab[-1]) + 0.37 * span)
            col[c == 8] = np.where(rs.random(rows) < 0.5, tab[0], tab[-1])[c == 8]
            col[c == 9] = (tab[0] + u * (tab[-1] - tab[0]))[c == 9]
        return out

    x = inputs(lambda f: knots[f])
    z = inputs(lambda f: levels)
    case = {"rows": rows, "D": D, "Q": Q, "kind": kind, "knots": knots, "levels": levels, "center": center, "scale": scale, "x": x, "z": z}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def reference(rows, D, Q, seed=0):
    """``(ref_forward(...), ref_inverse(...))`` of ``make_case(rows, D, Q, seed)``, computed once and shared."""
    c = make_case(rows, D, Q, seed)
    t = (c["kind"], c["knots"], c["levels"], c["center"], c["scale"])
    return ref_forward(c["x"], *t), ref_inverse(c["z"], *t)


# ---- the end-to-end cohort ------------------------------------------------------------------------------------------------------------
def write_cohort(root, n=200, n_mut=6, n_expr=30, n_path=4, seed=5):
    """The processed CSVs ``prepare_data`` reads, with zero-inflated log-expression: about 30 % exact zeros per gene, the rest
    log2(counts + 1) of a log-normal.  Returns the four frames."""
    import pandas as pd
    rs = np.random.RandomState(seed)
    ids = [f"TARGET-40-{i:04d}" for i in range(n)]
    root.mkdir(parents=True, exist_ok=True)
    mut = pd.DataFrame(rs.randint(0, 2, (n, n_mut)), index=ids, columns=[f"GENE{i}" for i in range(n_mut)])
    counts = np.floor(np.exp(rs.normal(4.0, 2.0, (n, n_expr))))
    counts[rs.random_sample((n, n_expr)) < 0.3] = 0.0
    expr = pd.DataFrame(np.log2(counts + 1.0), index=ids, columns=[f"EXPR{i}" for i in range(n_expr)])
    pw = pd.DataFrame(rs.randn(n, n_path) * 2.0 + 1.0, index=ids, columns=[f"HALLMARK_{i}" for i in range(n_path)])
    clin = pd.DataFrame({"submitter_id": ids, "survival_days": rs.randint(100, 2000, n), "event_occurred": rs.randint(0, 2, n),
                         "age_years": rs.uniform(10, 18, n), "metastasis_at_diagnosis": rs.randint(0, 2, n)})
    mut.to_csv(root / "mutation_matrix_aligned.csv")
    expr.to_csv(root / "expression_matrix_aligned.csv")
    pw.to_csv(root / "pathway_scores.csv")
    clin.to_csv(root / "clinical_aligned.csv", index=False)
    return mut, expr, pw, clin


def tiny_config(processed, save_dir, transform=None):
    """Dims 6 / 30 / 4, T = 10, hidden [32, 64, 32]."""
    data = {"processed_dir": str(processed)}
    if transform is not None:
        data["transform"] = dict(transform)
    return {"data": data,
            "model": {"architecture": "diffusion", "latent_dim": 128, "hidden_dims": [32, 64, 32], "gnn": {"dropout": 0.0},
                      "diffusion": {"num_steps": 10, "beta_schedule": "cosine"},
                      "condition_on": ["survival_time", "event_occurred", "age", "metastasis_at_diagnosis"]},
            "training": {"batch_size": 32, "num_epochs": 1, "learning_rate": 1e-3, "weight_decay": 1e-5, "patience": 100, "min_delta": 1e-4,
                         "augmentation": {"mixup_alpha": 0.0}, "val_split": 0.2, "random_seed": 42, "save_dir": str(save_dir),
                         "save_frequency": 1},
            "generation": {}}
