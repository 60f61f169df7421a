"""CPU: the float64 restatement of the GSEA permutation null (tests/gsea_helpers.py) and the package's host code above it
(osteosarcoma_diffusionmodel_amd/enrichment.py), driven over the NumPy stand-in.

  * every perm_ranks is a permutation; the k = 1 hit position at D = 16 over 4096 permutations (seed 7) is uniform: chi^2 = 17.45 on
    15 degrees of freedom, below the 99.9 % point 37.7; at D = 32768 the permutations 6, 9, 11, 13 and 15 hold one 32-bit key collision
    each, and the smaller index goes first;
  * es_pair against a plain loop over the whole list, weighted and unweighted, and the NR == 0 branch;
  * enrichment_statistics on hand-made arrays, enrichment_summary's NaN conventions, set selection, rank_positions' tie order;
  * planted signal (600 real, 900 synthetic patients, the 90 expression genes, the binary contrast, P = 1000, seed 7, weight 1):
    real UP NES +2.25 (p 0.0024), DOWN -2.29 (p 0.0018); faithful synthetic +2.28 / -2.24, nes_pearson 0.65; a synthetic cohort that
    ignores its condition (scale 0) UP -1.36, DOWN +1.63, nes_pearson -0.44."""
import functools

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import diffexp as DE
from osteosarcoma_diffusionmodel_amd import enrichment as EN
from diffexp_helpers import planted_cohort
from gsea_helpers import EXPR, WIDTHS, NumpyKernels, es_pair, gsea64, perm_keys, perm_ranks, planted_sets


# ---- the permutations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 5, 64, 1025])
def test_perm_ranks_are_permutations(D):
    assert np.array_equal(perm_ranks(7, 0, D), np.arange(D))
    seen = set()
    for p in range(1, 9):
        rho = perm_ranks(7, p, D)
        assert np.array_equal(np.sort(rho), np.arange(D))
        seen.add(tuple(rho))
    assert len(seen) > 1                                                            # the permutations differ from one another


def test_single_hit_position_is_uniform():
    D, P = 16, 4096
    counts = np.bincount([int(perm_ranks(7, p, D)[0]) for p in range(1, P + 1)], minlength=D)
    chi2 = float(((counts - P / D) ** 2 / (P / D)).sum())
    print(f"chi^2 = {chi2:.2f} on {D - 1} degrees of freedom")
    assert chi2 < 37.7


def test_key_collisions_go_to_the_smaller_index():
    D = 32768
    colliding = [p for p in range(1, 17) if np.unique(perm_keys(7, p, D)).size < D]
    assert colliding == [6, 9, 11, 13, 15]
    keys = perm_keys(7, 6, D)
    vals, cnt = np.unique(keys, return_counts=True)
    assert (cnt == 2).sum() == 1 and cnt.max() == 2
    a, b = np.flatnonzero(keys == vals[cnt == 2][0])
    rho = perm_ranks(7, 6, D)
    assert a < b and rho[b] == rho[a] + 1 and np.array_equal(np.sort(rho), np.arange(D))


# ---- the enrichment score ---------------------------------------------------------------------------------------------------------
def _walk(w, hits, D):
    """The running sum over the whole list, one position after another: (max, min) over all positions."""
    member = np.zeros(D, dtype=bool)
    member[hits] = True
    k, nr = int(member.sum()), float(w[member].sum())
    run, best, worst = 0.0, -np.inf, np.inf
    for i in range(D):
        run += (w[i] / nr if nr > 0 else 1.0 / k) if member[i] else -1.0 / (D - k)
        best, worst = max(best, run), min(worst, run)
    return best, worst


@pytest.mark.parametrize("weighted", [False, True])
def test_es_pair_is_the_running_sum(weighted):
    rs = np.random.default_rng(5)
    D = 200
    w = np.abs(rs.standard_normal(D)) if weighted else np.ones(D)
    for k in (1, 2, 17, 199):
        hits = rs.choice(D, k, replace=False)
        up, dn, ju, jd = es_pair(w, hits, D)
        best, worst = _walk(w, hits, D)
        # the walk rises at hits only and ends at 0: its maximum is at a hit and its minimum just before one, unless 0 beats them
        assert up - 1e-12 <= best <= max(up, 0.0) + 1e-12
        assert min(dn, 0.0) - 1e-12 <= worst <= dn + 1e-12
        assert 0 <= ju < k and 0 <= jd < k and -1.0 <= dn <= up <= 1.0
    # all hits first: ES+ = 1 at the last hit, ES- = 0 before the first one
    assert es_pair(np.ones(10), [2, 0, 1], 10) == (1.0, 0.0, 2, 0)
    # all hits last: ES- = -1 just before the first hit
    assert es_pair(np.ones(10), [9, 8, 7], 10)[1::2] == (-1.0, 0)
    # NR == 0: the unweighted ratios
    zero = es_pair(np.zeros(10), [1, 5, 6], 10)
    assert zero == es_pair(np.ones(10), [1, 5, 6], 10)
    r = gsea64(np.ones(10), [[0, 1, 2], [9, 8, 7]], 3, 7)
    assert r["es_pos"].shape == (4, 2) and r["lead"].tolist() == [[2, 0], [2, 0]] and r["es_pos"][0, 0] == 1.0 and r["es_neg"][0, 1] == -1.0


# ---- the host statistics ----------------------------------------------------------------------------------------------------------
def test_enrichment_statistics_on_hand_made_arrays():
    #              sign choice at a draw   ES = 0     no same-sign null   an ordinary set
    es_pos = np.array([[0.5, 0.0, 0.4, 0.6],
                       [0.2, 0.3, 0.1, 0.7],
                       [0.1, 0.0, 0.0, 0.2],
                       [0.6, 0.1, 0.05, 0.1],
                       [0.3, 0.2, 0.1, 0.3]])
    es_neg = np.array([[-0.5, 0.0, -0.1, -0.1],
                       [-0.4, -0.1, -0.5, -0.1],
                       [-0.3, 0.0, -0.6, -0.4],
                       [-0.1, -0.4, -0.7, -0.2],
                       [-0.3, -0.1, -0.2, -0.1]])
    lead = np.array([[2, 7], [0, 0], [4, 1], [5, 9]])
    sizes = np.array([10, 6, 8, 12])
    st = EN.enrichment_statistics(es_pos, es_neg, lead, sizes)
    assert st["es"].tolist() == [0.5, 0.0, 0.4, 0.6]                               # ES+ == -ES-: the positive one
    # set 0: nulls -0.4, -0.3, +0.6, +0.3 (a draw again): same sign 0.6, 0.3
    assert st["same_sign"].tolist() == [2, 4, 0, 2]
    assert st["nes"][0] == pytest.approx(0.5 / 0.45) and st["p"][0] == pytest.approx(2 / 3)
    # ES = 0: every null counts, every |null| >= 0
    assert st["nes"][1] == 0.0 and st["p"][1] == 1.0
    # no same-sign null: NES NaN, p = 1 / 1
    assert np.isnan(st["nes"][2]) and st["p"][2] == 1.0
    # set 3: nulls 0.7, -0.4, -0.2, 0.3: same sign 0.7, 0.3
    assert st["nes"][3] == pytest.approx(0.6 / 0.5) and st["p"][3] == pytest.approx(2 / 3)
    assert (st["p"] > 0).all() and np.array_equal(st["q"], DE.bh_qvalues(st["p"]))
    assert st["leading_edge"].tolist() == [3, 0, 5, 6]
    neg = EN.enrichment_statistics(-es_neg, -es_pos, lead, sizes)                  # the mirror image
    assert neg["es"].tolist() == [0.5, 0.0, -0.4, -0.6] and neg["leading_edge"].tolist() == [3, 0, 7, 3]
    # q is monotone in p
    p = np.array([0.001, 0.04, 0.03, 0.5, 0.5, 0.9])
    q = DE.bh_qvalues(p)
    assert (np.diff(q[np.argsort(p, kind="stable")]) >= 0).all() and (q >= p).all()
    only = EN.enrichment_statistics(es_pos[:1], es_neg[:1], lead, sizes)           # P = 0
    assert np.isnan(only["nes"]).all() and (only["p"] == 1.0).all()
    with pytest.raises(ValueError):
        EN.enrichment_statistics(es_pos, es_neg[:, :3], lead, sizes)


def _stats(nes, es, q):
    return {"nes": np.array(nes, dtype=np.float64), "es": np.array(es, dtype=np.float64), "q": np.array(q, dtype=np.float64)}


def test_enrichment_summary_and_its_nan_conventions():
    real = _stats([2.0, -2.0, 1.0, 0.5], [0.6, -0.6, 0.3, 0.1], [0.01, 0.01, 0.3, 0.9])
    same = EN.enrichment_summary(real, real)
    assert same["nes_pearson"] == pytest.approx(1.0) and same["nes_slope"] == pytest.approx(1.0) and same["nes_spearman"] == pytest.approx(1.0)
    assert (same["sign_agreement"], same["real_hits"], same["synth_hits"], same["precision"], same["recall"]) == (1.0, 2, 2, 1.0, 1.0)
    assert same["false_signal_share"] == 0.0 and same["max_abs_nes_gap"] == 0.0 and same["max_gap_set"] == 0
    flipped = _stats([-2.0, 2.0, 1.0, np.nan], [-0.6, 0.6, 0.3, 0.1], [0.01, 0.2, 0.3, 0.01])
    got = EN.enrichment_summary(real, flipped)
    assert got["sign_agreement"] == 0.0 and got["recall"] == 0.5 and got["precision"] == 0.5 and got["false_signal_share"] == 1.0
    assert got["max_abs_nes_gap"] == 4.0 and got["max_gap_set"] == 0              # the NaN set is left out of the NES figures
    assert got["nes_pearson"] == pytest.approx(EN.DE._pearson(np.array([2.0, -2.0, 1.0]), np.array([-2.0, 2.0, 1.0])))
    none = EN.enrichment_summary(_stats([1.0, 1.0], [0.3, 0.3], [0.6, 0.4]), _stats([np.nan, 0.5], [0.0, 0.2], [0.6, 0.7]))
    assert all(np.isnan(none[key]) for key in ("nes_pearson", "nes_spearman", "nes_slope", "sign_agreement", "precision", "recall"))
    assert none["false_signal_share"] == 0.0 and none["real_hits"] == 0 and none["max_abs_nes_gap"] == 0.5 and none["max_gap_set"] == 1
    gone = EN.enrichment_summary(_stats([np.nan], [0.0], [1.0]), _stats([np.nan], [0.0], [1.0]))
    assert np.isnan(gone["max_abs_nes_gap"]) and gone["max_gap_set"] == -1
    constant = EN.enrichment_summary(_stats([1.0, 1.0, 1.0], [0.3] * 3, [0.9] * 3), _stats([1.0, 2.0, 3.0], [0.3] * 3, [0.9] * 3))
    assert np.isnan(constant["nes_pearson"]) and np.isnan(constant["nes_slope"])


def test_set_selection_and_deduplication():
    import pandas as pd
    D = 12
    sets = {"dup": [3, 3, 1, 1, 7, 5, 9], "small": [0, 1], "all": list(range(12)), "most": list(range(11)), "six": [11, 0, 2, 4, 6, 8]}
    names, kept, skipped = EN.select_sets(sets, D, min_size=5, max_size=500)
    assert names == ["dup", "most", "six"] and skipped == 2                          # D - 1 members pass, D do not
    assert kept[0].tolist() == [1, 3, 5, 7, 9] and kept[2].tolist() == [0, 2, 4, 6, 8, 11]
    assert EN.select_sets(sets, D, min_size=5, max_size=6)[0] == ["dup", "six"]
    assert EN.select_sets(sets, D, min_size=1, max_size=4)[0] == ["small"]
    m = np.zeros((D, 3), dtype=np.int64)
    m[[1, 3, 5, 7, 9], 0] = 1
    m[:2, 1] = 1
    m[::2, 2] = 1
    names, kept, skipped = EN.select_sets(m, D, 5, 500)
    assert names == ["set0", "set2"] and skipped == 1 and kept[1].tolist() == [0, 2, 4, 6, 8, 10]
    frame = pd.DataFrame(m, columns=["P53", "TINY", "EVEN"], index=[f"G{i}" for i in range(D)])
    assert EN.select_sets(frame, D, 5, 500)[0] == ["P53", "EVEN"]
    # reindexed to the data's columns: absent genes drop out of their sets, unknown columns belong to none
    cols = [f"G{i}" for i in (9, 7, 5, 3, 1, 0)] + ["OTHER"]
    names, kept, skipped = EN.select_sets(frame, 7, 5, 500, columns=cols)
    assert names == ["P53"] and kept[0].tolist() == [0, 1, 2, 3, 4] and skipped == 2
    big = {"wide": list(range(1100))}
    assert EN.select_sets(big, 5000, 5, 5000) == ([], [], 1)                         # more than 1024 members
    for bad in ({"x": [0, 12]}, {"x": [-1, 2]}):
        with pytest.raises(ValueError):
            EN.select_sets(bad, D, 1, 500)
    with pytest.raises(ValueError):
        EN.select_sets(m[:5], D)
    with pytest.raises(ValueError):
        EN.select_sets(m * 2, D)
    with pytest.raises(ValueError):
        EN.select_sets(sets, D, min_size=0)


def test_rank_positions_tie_order_and_weights():
    stat = np.array([0.5, 2.0, 0.5, -1.0, 2.0, 0.0, -0.0, 0.5])
    pos = EN.rank_positions(stat)
    assert pos.tolist() == [2, 0, 3, 7, 1, 5, 6, 4]                                 # descending; equal values by ascending index
    w = EN.position_weights(stat, pos, 1.0)
    assert w.tolist() == [2.0, 2.0, 0.5, 0.5, 0.5, 0.0, 0.0, 1.0]
    assert EN.position_weights(stat, pos, 0.0).tolist() == [1.0] * 8                # 0 ** 0 = 1: the classic form
    assert EN.position_weights(stat, pos, 2.0)[7] == 1.0 and EN.position_weights(stat, pos, 2.0)[0] == 4.0
    with pytest.raises(ValueError):
        EN.rank_positions(np.array([1.0, np.nan]))


# ---- planted signal over the NumPy stand-in ---------------------------------------------------------------------------------------
SYNTH = {"faithful": dict(), "exaggerating": dict(scale=2.0), "ignoring": dict(scale=0.0)}


@functools.lru_cache(maxsize=None)
def _pipeline(sampler):
    (x, cr), (y, cs) = planted_cohort(600, 11, WIDTHS), planted_cohort(900, 12, WIDTHS, **SYNTH[sampler])
    names, sets, skipped = EN.select_sets(planted_sets(), 90, 5, 500)
    assert names == ["UP", "DOWN", "MIXED", "NULL_A", "NULL_B", "BIG", "SMALL"] and skipped == 0
    return EN.enrichment_metrics(NumpyKernels(), torch.from_numpy(x[:, EXPR]), cr[:, :1], torch.from_numpy(y[:, EXPR]), cs[:, :1],
                                 ["metastasis"], sets, 1.0, 1000, 0.05, 7, skipped)


def test_planted_sets_are_found_in_the_real_cohort():
    summary, rows = _pipeline("faithful")
    real, synth = rows["metastasis"]["real"], rows["metastasis"]["synthetic"]
    print("real NES", real["nes"], "p", real["p"], "\nsynthetic NES", synth["nes"])
    assert summary["gsea_real_hits_metastasis"] == 2 and (real["q"][:2] < 0.05).all() and (real["q"][2:] > 0.05).all()
    assert real["nes"][0] == pytest.approx(2.25, abs=0.005) and real["p"][0] == pytest.approx(0.0024, abs=5e-5)
    assert real["nes"][1] == pytest.approx(-2.29, abs=0.005) and real["p"][1] == pytest.approx(0.0018, abs=5e-5)
    assert synth["nes"][0] == pytest.approx(2.28, abs=0.005) and synth["nes"][1] == pytest.approx(-2.24, abs=0.005)
    assert summary["gsea_nes_pearson_metastasis"] == pytest.approx(0.65, abs=0.005)
    assert (summary["gsea_contrasts"], summary["gsea_skipped"], summary["gsea_sets"], summary["gsea_sets_skipped"]) == (1, 0, 7, 0)
    assert summary["gsea_recall_mean"] == summary["gsea_recall_metastasis"] and "gsea_real_hits_mean" not in summary
    assert (real["leading_edge"] >= 1).all() and (real["leading_edge"] <= real["size"]).all()
    assert real["es_pos"].shape == (1001, 7) and real["pos"].shape == (90,)


@pytest.mark.parametrize("sampler", ["faithful", "exaggerating"])
def test_a_cohort_that_follows_its_condition_agrees(sampler):
    summary = _pipeline(sampler)[0]
    assert summary["gsea_real_hits_metastasis"] == 2
    assert summary["gsea_sign_agreement_metastasis"] == 1 and summary["gsea_recall_metastasis"] == 1


def test_a_cohort_that_ignores_its_condition_does_not():
    summary, rows = _pipeline("ignoring")
    synth = rows["metastasis"]["synthetic"]
    assert synth["nes"][0] == pytest.approx(-1.36, abs=0.005) and synth["nes"][1] == pytest.approx(1.63, abs=0.005)
    assert summary["gsea_real_hits_metastasis"] == 2
    assert summary["gsea_sign_agreement_metastasis"] == 0 and summary["gsea_recall_metastasis"] == 0
    assert summary["gsea_nes_pearson_metastasis"] == pytest.approx(-0.44, abs=0.005)
    assert _pipeline("faithful")[0]["gsea_nes_pearson_metastasis"] > summary["gsea_nes_pearson_metastasis"] + 0.5


def test_a_contrast_with_an_empty_group_is_skipped():
    (x, cr), (y, cs) = planted_cohort(60, 11, WIDTHS), planted_cohort(70, 12, WIDTHS)
    sets = EN.select_sets(planted_sets(), 90, 5, 500)[1]
    cs = np.column_stack([np.ones(70), cs[:, 1]])
    summary, rows = EN.enrichment_metrics(NumpyKernels(), torch.from_numpy(x[:, EXPR]), cr, torch.from_numpy(y[:, EXPR]), cs,
                                          ["metastasis", "age"], sets, 0.0, 20, 0.05, 1, 3)
    assert (summary["gsea_contrasts"], summary["gsea_skipped"], summary["gsea_sets_skipped"]) == (1, 1, 3)
    assert "gsea_recall_age" in summary and "gsea_recall_metastasis" not in summary and list(rows) == ["age"]
    assert rows["age"]["threshold"] == float(np.median(cr[:, 1]))
