"""CPU: the host side of ``BiologicalValidator.differential_fidelity`` -- the int64 / float64 restatement of tests/diffexp_helpers.py
against scipy, ``diffexp.group_statistics`` against scipy's asymptotic Mann-Whitney test, the Benjamini-Hochberg q-values against
their definition, the float64 pipeline (``diffexp.differential_metrics`` over the NumPy stand-in) on planted cohorts, and the C ABI /
Python signatures."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import diffexp as DE
from diffexp_helpers import (ARRANGEMENTS, KINDS, NumpyKernels, arrange, group_ranks64, make_groups, planted_cohort, planted_effects)

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 1, 1), (1, 7, 5), (5, 3, 6), (64, 65, 9), (257, 130, 7), (130, 1031, 4)]


# ---- 1. the restatement against scipy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na,nb,D", SHAPES)
def test_restatement_equals_scipy(kind, na, nb, D):
    from scipy import stats
    a, b = make_groups(kind, na, nb, D)
    x, labels = arrange(a, b, "ignored")
    r = group_ranks64(x, labels)
    assert (r["na"], r["nb"]) == (na, nb)
    n = na + nb
    for f in range(D):
        af, bf = a[:, f].astype(np.float64), b[:, f].astype(np.float64)
        u = stats.mannwhitneyu(af, bf).statistic                            # U of the first sample, ties counted 1/2
        assert 2.0 * u == float(r["u2"][f])
        _, counts = np.unique(np.concatenate([af, bf]), return_counts=True)
        counts = counts.astype(np.int64)
        assert int(r["ties"][f]) == int((counts ** 3 - counts).sum())
    if kind == "all_equal":
        assert (r["u2"] == na * nb).all() and (r["ties"] == n ** 3 - n).all()
    if kind == "disjoint":
        assert (r["u2"][0::2] == 2 * na * nb).all() and (r["u2"][1::2] == 0).all()
    for how in ARRANGEMENTS:                                                # the arrangement of the rows changes nothing
        again = group_ranks64(*arrange(a, b, how))
        assert np.array_equal(again["u2"], r["u2"]) and np.array_equal(again["ties"], r["ties"])
        assert np.array_equal(again["sum"], r["sum"]) and np.array_equal(again["sumsq"], r["sumsq"])
    swapped = group_ranks64(x, np.where(labels == 1, 0, np.where(labels == 0, 1, labels)))
    assert np.array_equal(swapped["u2"], 2 * na * nb - r["u2"]) and np.array_equal(swapped["ties"], r["ties"])


@pytest.mark.parametrize("kind", ["continuous", "binary", "zero_inflated", "eight_values", "signed_zeros"])
@pytest.mark.parametrize("na,nb,D", [(5, 3, 6), (64, 65, 9), (257, 130, 7), (130, 1031, 4)])
def test_statistics_equal_scipy_asymptotic(kind, na, nb, D):
    from scipy import stats
    a, b = make_groups(kind, na, nb, D)
    x, labels = arrange(a, b, "alternating")
    s = DE.group_statistics(group_ranks64(x, labels))
    n = na + nb
    for f in range(D):
        af, bf = a[:, f].astype(np.float64), b[:, f].astype(np.float64)
        res = stats.mannwhitneyu(af, bf, use_continuity=False, method="asymptotic")
        ranks = stats.rankdata(np.concatenate([af, bf]))
        u1 = ranks[:na].sum() - na * (na + 1) / 2.0
        sd = np.sqrt(stats.tiecorrect(ranks) * na * nb * (n + 1) / 12.0)
        assert s["auc"][f] == res.statistic / (na * nb) and s["effect"][f] == 2.0 * s["auc"][f] - 1.0
        if sd == 0:                                                         # a constant feature: scipy divides 0 by 0
            assert s["z"][f] == 0.0 and s["p"][f] == 1.0
            continue
        z = (u1 - na * nb / 2.0) / sd
        assert abs(s["z"][f] - z) <= 1e-12 * max(abs(z), 1.0), (s["z"][f], z)
        assert abs(s["p"][f] - res.pvalue) <= 1e-12 * max(res.pvalue, 1e-300) + 1e-300, (s["p"][f], res.pvalue)


def test_bh_qvalues_equal_the_definition():
    rs = np.random.default_rng(5)
    for m in (1, 2, 17, 200):
        p = rs.random(m) ** 3
        p[rs.integers(0, m, m // 4)] = p[0]                                 # ties among the p-values
        order = np.sort(p)
        want = np.array([min(min(order[j] * m / (j + 1) for j in range(m) if order[j] >= pi), 1.0) for pi in p])
        assert np.array_equal(DE.bh_qvalues(p), want)
        assert (DE.bh_qvalues(p) >= p).all() and (np.diff(DE.bh_qvalues(p)[np.argsort(p, kind="stable")]) >= 0).all()
    assert np.array_equal(DE.bh_qvalues([1.0, 1.0, 1.0]), np.ones(3))
    assert np.array_equal(DE.bh_qvalues([0.01, 0.04, 0.03, 0.5]), np.array([0.04, 0.04 * 4 / 3, 0.04 * 4 / 3, 0.5]))


def test_moment_figures_and_constant_feature():
    rs = np.random.default_rng(9)
    a, b = rs.normal(1.0, 2.0, (40, 3)).astype(np.float32), rs.normal(0.0, 1.0, (70, 3)).astype(np.float32)
    a[:, 1], b[:, 1] = 2.5, 2.5                                             # constant over the pooled rows
    x, labels = arrange(a, b, "alternating")
    center = x.mean(0)
    s = DE.group_statistics(group_ranks64(x, labels, center))
    from scipy import stats
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for f in (0, 2):
        t = stats.ttest_ind(a64[:, f], b64[:, f], equal_var=False).statistic
        pooled = np.sqrt((39 * a64[:, f].var(ddof=1) + 69 * b64[:, f].var(ddof=1)) / 108.0)
        assert s["mean_diff"][f] == pytest.approx(a64[:, f].mean() - b64[:, f].mean(), rel=1e-12)
        assert s["welch_t"][f] == pytest.approx(t, rel=1e-10)
        assert s["cohen_d"][f] == pytest.approx((a64[:, f].mean() - b64[:, f].mean()) / pooled, rel=1e-10)
    assert s["effect"][1] == 0.0 and s["auc"][1] == 0.5 and s["z"][1] == 0.0 and s["p"][1] == 1.0 and s["q"][1] == 1.0
    assert s["welch_t"][1] == 0.0 and s["cohen_d"][1] == 0.0 and s["mean_diff"][1] == 0.0
    assert list(s) == list(DE.STAT_FIELDS)


# ---- 2. contrasts and the summary -------------------------------------------------------------------------------------------------
def test_contrast_labels_split_at_the_real_median():
    real, synth = np.array([3.0, 1.0, 2.0, 10.0, 7.0]), np.array([2.9, 3.0, 3.1, -5.0])
    lr, ls, thr = DE.contrast_labels(real, synth)
    assert thr == 3.0 and lr.tolist() == [0, 0, 0, 1, 1] and ls.tolist() == [0, 0, 1, 0]      # the REAL median, on both cohorts
    lr, ls, thr = DE.contrast_labels(np.array([0.0, 1.0, 1.0]), np.array([1.0, 0.0]))
    assert thr is None and lr.tolist() == [0, 1, 1] and ls.tolist() == [1, 0] and lr.dtype == np.int32
    lr, ls, thr = DE.contrast_labels(np.array([0.0, 1.0, 1.0]), np.array([1.0, 0.5]))      # not binary in the synthetic cohort
    assert thr == 1.0 and lr.tolist() == [0, 0, 0]


def test_contrast_summary_on_hand_made_rows():
    er = np.array([0.5, -0.4, 0.3, 0.0, 0.05, -0.02])
    qr = np.array([0.001, 0.01, 0.04, 0.9, 0.6, 0.7])
    es = np.array([0.25, 0.2, 0.15, 0.0, 0.3, -0.01])
    qs = np.array([0.01, 0.02, 0.2, 0.9, 0.03, 0.8])
    got = DE.contrast_summary({"effect": er, "q": qr}, {"effect": es, "q": qs}, alpha=0.05, top_k=2, bounds=[0, 3, 6], names=["a", "b"])
    assert got["real_hits"] == 3 and got["synth_hits"] == 3
    assert got["precision"] == 2 / 3 and got["recall"] == 2 / 3 and got["sign_agreement"] == 2 / 3
    assert got["topk_jaccard"] == 1 / 3                                     # {0, 1} against {4, 0}
    assert got["false_signal_share"] == 1 / 3                               # feature 4 of the three with real q > 0.5
    assert got["max_gap_feature"] == 1 and got["max_abs_effect_gap"] == pytest.approx(0.6)
    assert got["effect_slope"] == pytest.approx(np.polyfit(er, es, 1)[0]) and got["effect_pearson"] == pytest.approx(np.corrcoef(er, es)[0, 1])
    assert got["effect_pearson_a"] == pytest.approx(np.corrcoef(er[:3], es[:3])[0, 1]) and "effect_pearson_b" in got
    from scipy import stats
    assert got["effect_spearman"] == pytest.approx(stats.spearmanr(er, es)[0])
    none = DE.contrast_summary({"effect": er, "q": np.ones(6)}, {"effect": es, "q": np.ones(6)})
    assert none["real_hits"] == 0 and all(np.isnan(none[k]) for k in ("sign_agreement", "precision", "recall"))
    assert none["false_signal_share"] == 0.0 and "effect_pearson_a" not in none


# ---- 3. planted cohorts through the float64 pipeline ------------------------------------------------------------------------------
WIDTHS = (20, 180, 20)
N_REAL, N_SYNTH = 1200, 1500


def _pipeline(sampler):
    kw = {"faithful": {}, "ignoring": {"ignore": True}, "exaggerating": {"scale": 2.0}, "flipped": {"flip": True}}[sampler]
    x, cr = planted_cohort(N_REAL, 1, WIDTHS)
    y, cs = planted_cohort(N_SYNTH, 2, WIDTHS, **kw)
    return DE.differential_metrics(NumpyKernels(), torch.from_numpy(x), cr, torch.from_numpy(y), cs, ["metastasis", "age"],
                                   [0, 20, 200, 220], ["mutations", "expression", "pathways"])


def test_planted_cohorts_order_the_samplers():
    """Four samplers against one real cohort (1200 real and 1500 synthetic patients, 220 features; every fifth feature follows the
    binary condition, every seventh the continuous one).  Measured on the binary contrast, float64 pipeline:
        sampler        effect_slope  recall  sign_agreement  precision  effect_pearson
        faithful            0.912     0.930       0.977         0.930        0.887
        ignoring            0.049     0.000       0.651          nan         0.155
        exaggerating        1.595     0.977       0.977         0.933        0.918
        flipped             0.034     0.977       0.488         0.933        0.035
    and on the continuous contrast (effect_slope, recall): faithful 0.860, 0.886; ignoring -0.044, 0.000.
    Asserted, each an ordering that follows from the construction, with less than half the measured gap as margin: the slope of the
    exaggerating sampler over the faithful one by 0.3 (measured 0.68) and the faithful one over the ignoring one by 0.5 (0.86); recall
    above 0.8 against below 0.2; the flipped sampler's sign agreement within 0.1 of half the faithful one's (measured ratio 0.500)."""
    res = {name: _pipeline(name)[0] for name in ("faithful", "ignoring", "exaggerating", "flipped")}
    for name, r in res.items():
        print(name, {k: round(float(r[f"de_{k}_metastasis"]), 4) for k in ("effect_slope", "recall", "sign_agreement", "precision", "effect_pearson")},
              {k: round(float(r[f"de_{k}_age"]), 4) for k in ("effect_slope", "recall")})
    slope = {name: r["de_effect_slope_metastasis"] for name, r in res.items()}
    assert slope["exaggerating"] > slope["faithful"] + 0.3 and slope["faithful"] > slope["ignoring"] + 0.5
    assert res["faithful"]["de_recall_metastasis"] > 0.8 and res["ignoring"]["de_recall_metastasis"] < 0.2
    ratio = res["flipped"]["de_sign_agreement_metastasis"] / res["faithful"]["de_sign_agreement_metastasis"]
    assert abs(ratio - 0.5) < 0.1, ratio
    # the continuous contrast is split at the real median in both cohorts, and the faithful sampler keeps it too
    assert res["faithful"]["de_effect_slope_age"] > res["ignoring"]["de_effect_slope_age"] + 0.5
    assert res["faithful"]["de_recall_age"] > res["ignoring"]["de_recall_age"] + 0.5
    assert res["faithful"]["de_contrasts"] == 2 and res["faithful"]["de_skipped"] == 0
    means = [res["faithful"][f"de_effect_slope_{c}"] for c in ("metastasis", "age")]
    assert res["faithful"]["de_effect_slope_mean"] == pytest.approx(np.mean(means))


def test_planted_hits_are_the_planted_features():
    summary, rows = _pipeline("faithful")
    e0, e1 = planted_effects(WIDTHS)
    real = rows["metastasis"]["real"]
    hits = real["q"] < 0.05
    planted = e0 != 0
    assert hits[planted].mean() > 0.9 and hits[~planted].mean() < 0.1
    assert (np.sign(real["effect"][planted & hits]) == np.sign(e0[planted & hits])).all()
    assert rows["metastasis"]["threshold"] is None and rows["age"]["threshold"] == np.median(planted_cohort(N_REAL, 1, WIDTHS)[1][:, 1])
    assert summary["de_real_hits_metastasis"] == int(hits.sum())
    assert {"de_effect_pearson_mutations_metastasis", "de_effect_pearson_expression_age", "de_max_gap_feature_age"} <= set(summary)
    assert "de_max_gap_feature_mean" not in summary and "de_real_hits_mean" not in summary


def test_a_contrast_with_an_empty_group_is_skipped():
    x, cr = planted_cohort(200, 3, (4, 10, 4))
    y, cs = planted_cohort(300, 4, (4, 10, 4))
    cs = np.array(cs)
    cs[:, 0] = 1.0                                                          # no control in the synthetic cohort
    got, rows = DE.differential_metrics(NumpyKernels(), torch.from_numpy(x), cr, torch.from_numpy(y), cs, ["metastasis", "age"])
    assert got["de_skipped"] == 1 and got["de_contrasts"] == 1 and list(rows) == ["age"]
    assert not any(k.endswith("_metastasis") for k in got) and "de_effect_slope_age" in got
    cr2 = np.array(cr)
    cr2[:, 1] = 4.0                                                         # nothing above the real median
    got, rows = DE.differential_metrics(NumpyKernels(), torch.from_numpy(x), cr2, torch.from_numpy(y), cs, ["metastasis", "age"])
    assert got == {"de_contrasts": 0, "de_skipped": 2} and rows == {}


# ---- 4. the interface -------------------------------------------------------------------------------------------------------------
def test_signatures_and_declaration():
    from osteosarcoma_diffusionmodel_amd import _lib as L
    from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels
    header = (ROOT / "include" / "osdiff.h").read_text()
    m = re.search(r"int osd_val_group_ranks\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == len(L._SIGNATURES["osd_val_group_ranks"][1]) == 15
    assert len(L._SIGNATURES["osd_val_group_ranks_timed"][1]) == 16
    assert hasattr(L.lib(), "osd_val_group_ranks")
    assert list(inspect.signature(DeviceKernels.group_ranks).parameters)[:4] == ["self", "t", "labels", "center"]
    p = inspect.signature(BiologicalValidator.differential_fidelity).parameters
    assert list(p) == ["self", "real", "real_cond", "synthetic", "synth_cond", "names", "blocks", "alpha", "top_k", "return_rows"]
    assert (p["alpha"].default, p["top_k"].default, p["return_rows"].default, p["names"].default) == (0.05, 50, False, None)
    v = inspect.signature(BiologicalValidator.validate_all).parameters
    assert v["differential"].default is None and v["differential_names"].default is None
    doc = BiologicalValidator.differential_fidelity.__doc__
    assert "REAL cohort's median" in doc and "sharded" in doc


def test_bad_arguments_return_einval_before_any_device_call():
    import ctypes as C
    from osteosarcoma_diffusionmodel_amd import _lib as L
    lib = L.lib()
    out = [np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(8), np.zeros(8), np.zeros(1, dtype=np.int64),
           np.zeros(1, dtype=np.int64)]
    x = C.c_void_p(4096)                                                    # never dereferenced: the checks come first

    def call(X=x, rows=8, ld=4, D=4, labels=x, chunk=0, drop=None):
        ptrs = [None if i == drop else C.c_void_p(o.ctypes.data) for i, o in enumerate(out)]
        return lib.osd_val_group_ranks(None, 0, X, rows, ld, D, labels, None, chunk, *ptrs)

    for bad in [dict(X=None), dict(labels=None), dict(rows=0), dict(rows=-3), dict(D=0), dict(D=-1), dict(ld=3), dict(chunk=-1)] + \
            [dict(drop=i) for i in range(6)]:
        assert call(**bad) == L.OSD_EINVAL, bad
        assert L.last_error()
