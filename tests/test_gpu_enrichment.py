"""GPU: ``osd_val_gsea`` (csrc/gsea.hip: gs_ranks_sort / gs_ranks_count, gs_hits, gs_scan) and ``BiologicalValidator.enrichment_fidelity``
above it, against the float64 restatement of tests/gsea_helpers.py.

Kernel shapes (D; set sizes; P): (2; 1; 3), (5; 1, 4; 5), (64; 1, 63; 4), (65; 2, 64; 4), (257; 5, 255, 256; 4) -- the smallest lists,
sets of one and of all but one position, sizes around the wavefront and the workgroup width; (1025; 1 ... 1024; 3) a list just above a
power of two with every set size at which the hit kernels change their trip count; (5054; 29 overlapping sets of 5 ... 200 members, one
listed twice; 64); (32768; 1024, 7, 33, 1; 16) the largest list: 128 KiB of keys, and permutation 6 of seed 7 holds one 32-bit key
collision -- the set of 7 holds the colliding pair's smaller index only, the sets of 33 and of 1 the larger one only, whose rank the
tie order decides.
Five kinds of weights: continuous, all ones, 30 % zeros with the smallest set wholly on zeros (NR == 0 in row 0), all zero (NR == 0
everywhere), magnitudes from 1e-100 to 1e100.

  * es_pos and es_neg are BIT-EQUAL to the restatement and lead is equal, with either rank kernel;
  * perm_chunk 0, 1, 7 and P, a repeated call and the timed twin: identical bits; another seed changes the null rows and not row 0;
  * every OSD_EINVAL case, D = 32768 passes and D = 32769 is refused; the wrapper's ValueErrors.

End to end (600 real and 900 synthetic patients, the 90 expression genes, seven planted sets, P = 1000, seed 7): every summary key and
the per-set ES, NES, p, q and leading-edge size EQUAL the float64 pipeline -- the package's own host code over the NumPy stand-in: the
ranking z derives from integers and the ES are bit-equal, so there is no tolerance."""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import enrichment as EN
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels
from diffexp_helpers import planted_cohort
from gsea_helpers import EXPR, WIDTHS, NumpyKernels, es_pair, gsea64, perm_keys, perm_ranks, planted_sets

pytestmark = pytest.mark.gpu

SEED = 7
SHAPES = {
    "d2": (2, (1,), 3),
    "d5": (5, (1, 4), 5),
    "d64": (64, (1, 63), 4),
    "d65": (65, (2, 64), 4),
    "d257": (257, (5, 255, 256), 4),
    "d1025": (1025, (1, 2, 63, 64, 65, 255, 256, 257, 1024), 3),
    "d5054": (5054, None, 64),
    "d32768": (32768, None, 16),
    "d257_one_set": (257, (40,), 4),
    "d257_300_sets": (257, tuple(1 + (7 * s) % 120 for s in range(300)), 4),
    "no_permutation": (257, (5, 255, 256), 0),
}
KINDS = ["continuous", "ones", "zero_inflated", "all_zero", "spread"]
CONF = {"evaluation": {}}


def _collision(D=32768, p=6):
    """(a, b), a < b: the two positions of permutation p whose keys collide; asserted to exist, on the reference side."""
    keys = perm_keys(SEED, p, D)
    vals, cnt = np.unique(keys, return_counts=True)
    assert (cnt == 2).sum() == 1 and cnt.max() == 2, "permutation 6 of seed 7 holds exactly one key collision at D = 32768"
    a, b = np.flatnonzero(keys == vals[cnt == 2][0])
    rho = perm_ranks(SEED, p, D)
    assert a < b and rho[b] == rho[a] + 1
    return int(a), int(b)


def _sets(name, D, sizes, rs):
    if name == "d5054":                                        # a pool of 700 positions: the sets overlap heavily; set 3 comes twice
        pool = rs.choice(D, 700, replace=False)
        sets = [rs.choice(pool, int(k), replace=False) for k in np.linspace(5, 200, 28).astype(int)]
        return sets + [sets[3].copy()]
    if name == "d32768":
        a, b = _collision()
        rest = np.setdiff1d(np.arange(D), [a, b])
        return [rs.choice(D, 1024, replace=False), np.append(rs.choice(rest, 6, replace=False), a),
                np.append(rs.choice(rest, 32, replace=False), b), np.array([b])]
    return [rs.choice(D, k, replace=False) for k in sizes]


def _weights(kind, D, sets, rs):
    if kind == "continuous":
        return np.abs(rs.standard_normal(D)) * 3.0
    if kind == "ones":
        return np.ones(D)
    if kind == "all_zero":
        return np.zeros(D)
    if kind == "spread":
        return 10.0 ** rs.uniform(-100.0, 100.0, D)
    if kind != "zero_inflated":
        raise ValueError(kind)
    w = np.where(rs.random(D) < 0.3, 0.0, np.abs(rs.standard_normal(D)))
    small = min(range(len(sets)), key=lambda s: len(sets[s]))
    w[sets[small]] = 0.0                                       # the smallest set sits wholly on zeros: NR == 0 in row 0
    return w


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    D, sizes, P = SHAPES[name]
    rs = np.random.default_rng(1000 * list(SHAPES).index(name) + KINDS.index(kind))
    sets = _sets(name, D, sizes, np.random.default_rng(list(SHAPES).index(name)))
    w = _weights(kind, D, sets, rs)
    return w, sets, P, gsea64(w, sets, P, SEED)


def _kernels():
    return DeviceKernels(torch.device("cuda:0"))


def _same_bits(got, ref, what=""):
    for name in ("es_pos", "es_neg"):
        assert got[name].dtype == np.float64 and got[name].shape == ref[name].shape, (name, what)
        diff = got[name].view(np.int64) != ref[name].view(np.int64)
        assert not diff.any(), (name, what, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert got["lead"].dtype == np.int32 and np.array_equal(got["lead"], ref["lead"]), ("lead", what)


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_gsea_bit_equal_to_restatement(name, kind):
    w, sets, P, ref = _case(name, kind)
    got = _kernels().gsea(w, sets, P, SEED)
    assert got["es_pos"].shape == (P + 1, len(sets)) and got["lead"].shape == (len(sets), 2)
    _same_bits(got, ref, (name, kind))
    if kind == "zero_inflated":
        small = min(range(len(sets)), key=lambda s: len(sets[s]))
        assert w[sets[small]].sum() == 0.0                      # row 0 of that set went through the NR == 0 branch


@pytest.mark.parametrize("name,kind", [("d5", "continuous"), ("d65", "spread"), ("d1025", "zero_inflated"), ("d5054", "continuous"),
                                       ("d32768", "continuous"), ("d257_300_sets", "ones")])
def test_gsea_counting_rank_kernel_gives_the_same_bits(name, kind, monkeypatch):
    w, sets, P, ref = _case(name, kind)
    monkeypatch.setenv("OSD_GSEA_RANKS", "count")
    _same_bits(_kernels().gsea(w, sets, P, SEED), ref, (name, kind, "count"))


def test_gsea_collision_decides_a_rank():
    """Without the tie order the set that holds the larger colliding index would get the smaller one's rank in permutation 6."""
    a, b = _collision()
    w, sets, P, ref = _case("d32768", "continuous")
    assert a in sets[1] and b not in sets[1] and b in sets[2] and a not in sets[2] and sets[3].tolist() == [b] and P >= 6
    rho = perm_ranks(SEED, 6, 32768)
    wrong = rho.copy()
    wrong[b] = rho[a]
    assert es_pair(w, wrong[sets[3]], 32768)[0] != es_pair(w, rho[sets[3]], 32768)[0] == ref["es_pos"][6, 3]      # the score depends on it
    _same_bits(_kernels().gsea(w, sets, P, SEED), ref, "collision")


@pytest.mark.parametrize("name,kind,P", [("d257", "continuous", 20), ("d5054", "zero_inflated", 64)])
def test_gsea_same_bits_at_every_chunk_call_and_twin(name, kind, P):
    w, sets, _, _ = _case(name, kind)
    k = _kernels()
    first = k.gsea(w, sets, P, SEED)
    _same_bits(first, gsea64(w, sets, P, SEED) if name == "d257" else _case(name, kind)[3], "reference")
    for chunk in (0, 1, 7, P, P + 1, 100000):
        _same_bits(k.gsea(w, sets, P, SEED, perm_chunk=chunk), first, chunk)
    _same_bits(k.gsea(w, sets, P, SEED), first, "repeated")
    timed = k.gsea(w, sets, P, SEED, perm_chunk=7, phases=True)
    _same_bits(timed, first, "timed")
    assert timed["phase_ms"].shape == (3,) and (timed["phase_ms"] >= 0).all() and timed["phase_ms"].sum() > 0
    other = k.gsea(w, sets, P, SEED + 1)
    assert np.array_equal(other["es_pos"][0].view(np.int64), first["es_pos"][0].view(np.int64))
    assert np.array_equal(other["es_neg"][0].view(np.int64), first["es_neg"][0].view(np.int64)) and np.array_equal(other["lead"], first["lead"])
    assert (other["es_pos"][1:] != first["es_pos"][1:]).any() and (other["es_neg"][1:] != first["es_neg"][1:]).any()
    shuffled = [np.random.default_rng(3).permutation(m) for m in sets]          # the members of a set come in any order
    _same_bits(k.gsea(w, shuffled, P, SEED), first, "members shuffled")


def test_gsea_argument_errors():
    lib = L.lib()
    D, S, P = 16, 2, 3
    w = np.ones(D)
    off, pos = np.array([0, 3, 8], dtype=np.int32), np.array([0, 5, 9, 1, 2, 3, 4, 15], dtype=np.int32)
    out = [np.zeros((P + 1, S)), np.zeros((P + 1, S)), np.zeros((S, 2), dtype=np.int32)]
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ptr(a):
        return None if a is None else C_.c_void_p(a.ctypes.data)

    def call(w=w, D=D, off=off, pos=pos, S=S, P=P, chunk=0, drop=None, timed=None):
        outs = [None if i == drop else ptr(o) for i, o in enumerate(out)]
        if timed is not None:
            return lib.osd_val_gsea_timed(stream, 0, ptr(w), D, ptr(off), ptr(pos), S, P, SEED, chunk, *outs, timed[0])
        return lib.osd_val_gsea(stream, 0, ptr(w), D, ptr(off), ptr(pos), S, P, SEED, chunk, *outs)

    def arr(v):
        return np.array(v, dtype=np.int32)

    def weights(i, v):
        bad = np.ones(D)
        bad[i] = v
        return bad

    assert call() == L.OSD_OK and call(chunk=2) == L.OSD_OK and call(P=0) == L.OSD_OK
    ms = (C_.c_float * 3)()
    assert call(timed=[ms]) == L.OSD_OK and all(v >= 0 for v in ms)
    assert call(w=weights(4, 1e100)) == L.OSD_OK
    wide = arr(np.arange(15))                                  # k = D - 1 passes, k = D does not
    assert call(off=arr([0, 15]), pos=wide, S=1) == L.OSD_OK
    cases = [dict(w=None), dict(off=None), dict(pos=None), dict(drop=0), dict(drop=1), dict(drop=2), dict(timed=[None]),
             dict(D=1), dict(D=0), dict(D=-3), dict(S=0), dict(S=-1), dict(P=-1), dict(chunk=-1),
             dict(off=arr([0, 0, 8])), dict(off=arr([0, 8, 3])), dict(off=arr([1, 3, 8])),                 # an empty set, k < 0, a start off 0
             dict(off=arr([0, 16]), pos=arr(np.arange(16)), S=1),                                              # k == D
             dict(pos=arr([0, 5, 16, 1, 2, 3, 4, 15])), dict(pos=arr([0, 5, -1, 1, 2, 3, 4, 15])),            # outside [0, D)
             dict(pos=arr([0, 5, 5, 1, 2, 3, 4, 15])), dict(pos=arr([0, 5, 9, 1, 2, 3, 1, 15])),              # repeated inside a set
             dict(w=weights(3, -1e-300)), dict(w=weights(0, np.nan)), dict(w=weights(15, np.inf)), dict(w=weights(7, 1.0001e100))]
    for bad in cases:
        assert call(**bad) == L.OSD_EINVAL, bad
        assert L.last_error(), bad
    assert call(pos=arr([0, 5, 9, 0, 5, 9, 4, 15])) == L.OSD_OK                    # the same position in two sets is no repeat
    big_w, big_set = np.ones(2000), arr(np.arange(1025))
    assert call(w=big_w, D=2000, off=arr([0, 1025]), pos=big_set, S=1) == L.OSD_EINVAL and "1024" in L.last_error()
    assert call(w=big_w, D=2000, off=arr([0, 1024]), pos=big_set, S=1) == L.OSD_OK
    one = arr([32767])
    assert call(w=np.ones(32768), D=32768, off=arr([0, 1]), pos=one, S=1) == L.OSD_OK
    assert call(w=np.ones(32769), D=32769, off=arr([0, 1]), pos=one, S=1) == L.OSD_EINVAL and "32768" in L.last_error()

    k = _kernels()
    good = [[0, 5, 9], [1, 2, 3, 4, 15]]
    assert k.gsea(w, good, 2, SEED)["es_pos"].shape == (3, 2)
    for bad in [dict(set_positions=[]), dict(permutations=-1), dict(perm_chunk=-1), dict(weights=np.ones(1), set_positions=[[0]]),
                dict(set_positions=[[0, 16]]), dict(set_positions=[[3, 3]]), dict(set_positions=[[]]), dict(set_positions=[list(range(16))]),
                dict(weights=weights(2, -1.0)), dict(weights=weights(2, np.nan)), dict(weights=np.ones((4, 4))),
                dict(set_positions=[[2 ** 40]])]:
        args = dict(weights=w, set_positions=good, permutations=2, seed=SEED)
        args.update(bad)
        with pytest.raises(ValueError):
            k.gsea(**args)


# ---- 2. enrichment_fidelity end to end --------------------------------------------------------------------------------------------
N_REAL, N_SYNTH = 600, 900
NAMES = ["metastasis", "age"]
SAMPLERS = {"faithful": dict(), "ignoring": dict(scale=0.0)}


@functools.lru_cache(maxsize=None)
def _cohorts(sampler="faithful"):
    return planted_cohort(N_REAL, 11, WIDTHS), planted_cohort(N_SYNTH, 12, WIDTHS, **SAMPLERS[sampler])


@functools.lru_cache(maxsize=None)
def _pipeline64(sampler):
    (x, cr), (y, cs) = _cohorts(sampler)
    names, sets, skipped = EN.select_sets(planted_sets(), 90, 5, 500)
    return EN.enrichment_metrics(NumpyKernels(), torch.from_numpy(x[:, EXPR]), cr, torch.from_numpy(y[:, EXPR]), cs, NAMES, sets, 1.0,
                                 1000, 0.05, SEED, skipped)


@functools.lru_cache(maxsize=None)
def _device(sampler="faithful"):
    (x, cr), (y, cs) = _cohorts(sampler)
    return BiologicalValidator(CONF).enrichment_fidelity(x[:, EXPR], cr, y[:, EXPR], cs, planted_sets(), names=NAMES, permutations=1000,
                                                         seed=SEED, return_rows=True)


def _equal(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_enrichment_fidelity_equals_float64_pipeline(sampler):
    (got, rows), (want, rows64) = _device(sampler), _pipeline64(sampler)
    assert list(got) == list(want) and got["gsea_contrasts"] == 2 and got["gsea_skipped"] == 0
    assert got["gsea_sets"] == 7 and got["gsea_sets_skipped"] == 0 and rows["sets"] == list(planted_sets())
    for key, w in want.items():
        assert _equal(got[key], w), (key, got[key], w)
    for name in NAMES:
        assert rows[name]["threshold"] == rows64[name]["threshold"]
        for cohort in ("real", "synthetic"):
            d, h = rows[name][cohort], rows64[name][cohort]
            for field in ("stat", "pos", "size", "es", "nes", "p", "q", "leading_edge", "same_sign", "es_pos", "es_neg"):
                assert np.array_equal(d[field], h[field], equal_nan=True), (name, cohort, field)


def test_enrichment_fidelity_reads_the_planted_signal():
    faithful, ignoring = _device("faithful")[0], _device("ignoring")[0]
    assert faithful["gsea_real_hits_metastasis"] == 2 == ignoring["gsea_real_hits_metastasis"]
    assert faithful["gsea_sign_agreement_metastasis"] == 1 and faithful["gsea_recall_metastasis"] == 1
    assert ignoring["gsea_sign_agreement_metastasis"] == 0 and ignoring["gsea_recall_metastasis"] == 0
    assert faithful["gsea_nes_pearson_metastasis"] > ignoring["gsea_nes_pearson_metastasis"] + 0.5
    assert 0 <= faithful["gsea_max_gap_set_metastasis"] < 7


def test_validate_all_carries_the_enrichment_keys():
    import pandas as pd
    (x, cr), (y, cs) = _cohorts()

    def frames(a):
        mut = pd.DataFrame(a[:, :20], columns=[f"M{i}" for i in range(20)])
        expr = pd.DataFrame(a[:, 20:110], columns=[f"G{i}" for i in range(90)])
        pw = pd.DataFrame(a[:, 110:], columns=[f"PW{i}" for i in range(20)])
        return mut, expr, pw

    sets = planted_sets()
    genes = [f"G{i}" for i in range(90)]
    rows = ["ABSENT_A"] + genes[::-1] + ["ABSENT_B"]           # another order than the expression columns, and two genes they lack
    pgm = pd.DataFrame(0, index=rows, columns=list(sets))
    for name, members in sets.items():
        pgm.loc[[genes[i] for i in members], name] = 1
    pgm.loc["ABSENT_A", "UP"] = pgm.loc["ABSENT_B", "SMALL"] = 1
    val = BiologicalValidator(CONF)
    np.random.seed(5)
    plain = val.validate_all(*frames(x), *frames(y), pathway_gene_matrix=pgm)
    np.random.seed(5)
    full = val.validate_all(*frames(x), *frames(y), pathway_gene_matrix=pgm, enrichment=(cr, cs), enrichment_names=NAMES,
                            enrichment_permutations=200)
    assert not any(k.startswith("gsea_") for k in plain)
    extra = [k for k in full if k not in plain]
    assert all(k.startswith("gsea_") for k in extra) and [k for k in full if k in plain] == list(plain)
    assert all(full[k] == pytest.approx(plain[k], rel=1e-9, abs=1e-12, nan_ok=True) for k in plain)      # double atomics: last-bit freedom
    direct = val.enrichment_fidelity(x[:, EXPR], cr, y[:, EXPR], cs, sets, names=NAMES, permutations=200)
    assert extra == list(direct) and all(_equal(full[k], direct[k]) for k in extra)
    assert full["gsea_sets"] == 7 and full["gsea_real_hits_metastasis"] >= 1
    named = val.validate_all(*frames(x), *frames(y), pathway_gene_matrix=pgm, enrichment=(pd.DataFrame(cr, columns=NAMES), cs),
                             enrichment_permutations=50)
    assert [k for k in named if k.startswith("gsea_")] == extra
    with pytest.raises(ValueError):
        val.validate_all(*frames(x), *frames(y), pathway_gene_matrix=pgm, enrichment=(cr,))
    with pytest.raises(ValueError):
        val.validate_all(*frames(x), *frames(y), enrichment=(cr, cs))


def test_enrichment_fidelity_set_forms_argument_errors_and_shards():
    (x, cr), (y, cs) = _cohorts()
    x, y = x[:, EXPR], y[:, EXPR]
    val = BiologicalValidator(CONF)
    sets = planted_sets()
    base = val.enrichment_fidelity(x, cr, y, cs, sets, names=NAMES, permutations=100, seed=SEED)
    m = np.zeros((90, len(sets)), dtype=np.int64)
    for s, members in enumerate(sets.values()):
        m[members, s] = 1
    as_matrix = val.enrichment_fidelity(x, cr, y, cs, m, names=NAMES, permutations=100, seed=SEED)
    assert list(as_matrix) == list(base) and all(_equal(as_matrix[k], base[k]) for k in base)
    doubled = {name: np.concatenate([members, members[::-1]]) for name, members in sets.items()}       # members are de-duplicated
    again = val.enrichment_fidelity(x, cr, y, cs, doubled, names=NAMES, permutations=100, seed=SEED)
    assert all(_equal(again[k], base[k]) for k in base)
    fewer = val.enrichment_fidelity(x, cr, y, cs, sets, names=NAMES, permutations=100, seed=SEED, min_size=6, max_size=12)
    assert fewer["gsea_sets"] == 5 and fewer["gsea_sets_skipped"] == 2               # SMALL (5) and BIG (40) are dropped
    classic = val.enrichment_fidelity(x, cr, y, cs, sets, names=NAMES, permutations=100, seed=SEED, weight=0.0)
    assert classic["gsea_real_hits_metastasis"] >= 1
    skipped = val.enrichment_fidelity(x, cr, y, np.column_stack([np.ones(N_SYNTH), cs[:, 1]]), sets, names=NAMES, permutations=20)
    assert skipped["gsea_skipped"] == 1 and skipped["gsea_contrasts"] == 1 and "gsea_recall_age" in skipped
    assert "gsea_recall_metastasis" not in skipped
    bad = np.array(x)
    bad[3, 7] = np.nan
    with pytest.raises(ValueError, match="real"):
        val.enrichment_fidelity(bad, cr, y, cs, sets)
    with pytest.raises(ValueError, match="synthetic"):
        val.enrichment_fidelity(x, cr, y[:, :80], cs, sets)
    with pytest.raises(ValueError, match="synthetic"):
        val.enrichment_fidelity(x, cr, y, cs[:-1], sets)
    for kw in (dict(names=["only_one"]), dict(alpha=0.0), dict(permutations=-1), dict(weight=-1.0), dict(min_size=50),
               dict(min_size=0)):
        with pytest.raises(ValueError):
            val.enrichment_fidelity(x, cr, y, cs, sets, **kw)
    with pytest.raises(ValueError):
        val.enrichment_fidelity(x, cr, y, cs, {"x": [0, 1, 2, 3, 90]})
    sharded = BiologicalValidator(CONF, sharded=True)
    with pytest.raises(ValueError, match="shard"):
        sharded.enrichment_fidelity(x, cr, y, cs, sets)
