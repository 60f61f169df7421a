"""CPU: the host side of pathway scoring and of ``BiologicalValidator.pathway_consistency`` (osteosarcoma_diffusionmodel_amd/pathways.py)
over the float64 stand-in of tests/pathway_helpers.py -- GMT files, name resolution, the closed form of the ssGSEA score against the
literal walk, reference parity of ``mean`` on a fixture the reference made (tests/golden/make_pathway_golden.py), the planted
consistency design, a sharded run over gloo, ``prepare_data`` with and without ``data.gene_sets_file``, and the argument errors."""
import inspect
import os
import socket

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pathway_helpers import N_GENES, N_SYNTH, U53, NumpyKernels, literal_walk, planted_cohorts, rank_table, ssgsea64
from osteosarcoma_diffusionmodel_amd import pathways as PW


def scorer(sets, genes, **kw):
    return PW.PathwayScorer(sets, genes, kernels=NumpyKernels(), **kw)


# ---- 1. GMT -----------------------------------------------------------------------------------------------------------------------
def test_gmt_round_trip_blank_descriptions_and_duplicate_members(tmp_path):
    sets = {"HALLMARK_A": ["TP53", "MDM2", "BAX"], "B set": ["G1"], "C": ["X", "Y", "Z", "W", "V", "U"]}
    path = tmp_path / "sets.gmt"
    PW.write_gmt(sets, path)
    text = path.read_text()
    assert text.splitlines()[0] == "HALLMARK_A\t\tTP53\tMDM2\tBAX"                 # a blank description column
    back = PW.read_gmt(path)
    assert back == sets and list(back) == list(sets)
    path.write_text("S1\tsome words\tA\tB\tA\t\tC\r\n\nS2\t\tD\n")                  # a duplicate member, an empty cell, a blank line
    assert PW.read_gmt(path) == {"S1": ["A", "B", "C"], "S2": ["D"]}
    PW.write_gmt(sets, path, descriptions={"C": "the third"})
    assert path.read_text().splitlines()[2].split("\t")[:3] == ["C", "the third", "X"] and PW.read_gmt(path) == sets
    path.write_text("S1\t\tA\nS1\t\tB\n")
    with pytest.raises(ValueError, match="twice"):
        PW.read_gmt(path)
    path.write_text("lonely\n")
    with pytest.raises(ValueError):
        PW.read_gmt(path)
    with pytest.raises(ValueError):
        PW.write_gmt({"S": ["A\tB"]}, path)


# ---- 2. name resolution -----------------------------------------------------------------------------------------------------------
def test_name_resolution_min_genes_and_the_order_of_names():
    genes = [f"G{i}" for i in range(12)]
    sets = {"LATE": ["G9", "G3", "G5", "G7", "G1", "G3"],                # six listed, five distinct: kept, in the order of the listing
            "THIN": ["G0", "G1", "G2", "G4", "ABSENT1", "ABSENT2"],      # four present: dropped at min_genes = 5
            "EARLY": ["G0", "G1", "G2", "G4", "G6", "NOPE"],
            "NONE": ["Q", "R"]}
    s = scorer(sets, genes)
    assert s.names == ["LATE", "EARLY"] and s.skipped == 2 and s.skipped_names == ["THIN", "NONE"]
    assert [m.tolist() for m in s.sets] == [[9, 3, 5, 7, 1], [0, 1, 2, 4, 6]]
    assert scorer(sets, genes, min_genes=4).names == ["LATE", "THIN", "EARLY"]
    with pytest.raises(ValueError, match="no gene set"):
        scorer(sets, genes, min_genes=7)
    # column indices and a genes x sets 0/1 frame name the same sets (members sorted there)
    by_index = scorer({"LATE": [9, 3, 5, 7, 1], "THIN": [0, 1, 2, 4], "EARLY": [0, 1, 2, 4, 6]}, genes)
    assert by_index.names == ["LATE", "EARLY"] and [m.tolist() for m in by_index.sets] == [[1, 3, 5, 7, 9], [0, 1, 2, 4, 6]]
    frame = PW.gene_pathway_matrix(sets)
    by_frame = scorer(frame, genes)
    assert by_frame.names == ["LATE", "EARLY"] and by_frame.skipped == 2
    assert [m.tolist() for m in by_frame.sets] == [m.tolist() for m in by_index.sets]
    x = np.random.default_rng(0).random((4, 12)).astype(np.float32)
    assert np.allclose(s.score(x).numpy(), by_frame.score(x).numpy(), rtol=1e-14, atol=0)       # the same sets in another order
    with pytest.raises(ValueError):
        scorer(sets, genes, method="gsva")
    with pytest.raises(ValueError):
        scorer(sets, genes[:1])


# ---- 3. the closed form against the literal walk ----------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("D,m", [(2, 1), (5, 4), (64, 63), (257, 40), (5054, 200)])
def test_closed_form_equals_the_literal_walk(D, m, alpha):
    rs = np.random.default_rng(1000 * D + m)
    x = rs.permutation(D).astype(np.float32) * 0.37 - 11.0        # untied
    assert np.unique(x).size == D
    members = rs.permutation(D)[:m]
    closed = ssgsea64(x[None, :], [members], rank_table(D, alpha))[0, 0]
    walk = literal_walk(x, members, alpha)
    print(f"D={D} m={m} alpha={alpha}: closed {closed!r} walk {walk!r} diff {abs(closed - walk):.3e}")
    assert abs(closed - walk) <= 4 * U53 * D * (m + 4)
    via_scorer = scorer({"s": members}, list(range(D)), method="ssgsea", alpha=alpha, min_genes=1).score(x[None, :]).numpy()[0, 0]
    assert abs(via_scorer - closed) <= 4 * U53 * D * (m + 4)                     # the scorer sorts an index set's members


def test_ties_do_not_depend_on_the_order_of_equal_values():
    rs = np.random.default_rng(5)
    D = 300
    x = np.where(rs.random(D) < 0.3, 0.0, rs.gamma(2.0, 1.5, D)).astype(np.float32)
    x[np.flatnonzero(x == 0)[0]] = -0.0
    assert np.signbit(x).sum() == 1 and (x == 0).sum() > 50
    sets = [rs.permutation(D)[:m] for m in (5, 40, 299)]
    table = rank_table(D)
    base = ssgsea64(x[None, :], sets, table)
    for trial in range(3):
        perm = rs.permutation(D)
        inv = np.empty(D, dtype=np.int64)
        inv[perm] = np.arange(D)
        moved = ssgsea64(x[perm][None, :], [inv[m] for m in sets], table)
        assert np.array_equal(base.view(np.int64), moved.view(np.int64))
    assert np.isnan(ssgsea64(np.where(np.arange(D) == 7, np.nan, x)[None, :], sets, table)).all()


# ---- 4. reference parity for `mean` -----------------------------------------------------------------------------------------------
def _golden(golden_dir):
    g = dict(np.load(golden_dir / "g11_pathway_scores.npz"))
    names, off = [str(n) for n in g["set_names"]], g["set_offsets"]
    g["gene_sets"] = {n: [str(s) for s in g["set_members"][off[i]:off[i + 1]]] for i, n in enumerate(names)}
    return g


def test_mean_reproduces_the_reference(golden_dir):
    g = _golden(golden_dir)
    columns, patients = [str(c) for c in g["columns"]], [str(p) for p in g["patients"]]
    assert g["expression"].shape == (40, 300) and len(g["gene_sets"]) == 29
    s = scorer(g["gene_sets"], columns)
    assert s.names == [str(n) for n in g["score_names"]]                         # the kept sets, in the reference's column order
    assert s.skipped_names == [n for n in g["gene_sets"] if n not in set(s.names)] and s.skipped == 2
    expression = pd.DataFrame(g["expression"], index=patients, columns=columns)
    got = s.score(expression)
    assert list(got.columns) == s.names and list(got.index) == patients
    x64 = g["expression"].astype(np.float64)
    for q, m in enumerate(s.sets):
        bound = 2 * (len(m) + 4) * U53 * np.abs(x64[:, m]).sum(axis=1) / len(m)
        assert (np.abs(got.values[:, q] - g["scores"][:, q]) <= bound).all(), s.names[q]
    mutations = pd.DataFrame(g["mutations"], index=patients, columns=columns)
    burden = scorer(g["gene_sets"], columns).score(mutations)
    assert list(burden.columns) == [str(n) for n in g["burden_names"]]
    m64 = g["mutations"].astype(np.float64)
    for q, m in enumerate(s.sets):
        bound = 2 * (len(m) + 4) * U53 * np.abs(m64[:, m]).sum(axis=1) / len(m)
        assert (np.abs(burden.values[:, q] - g["burden"][:, q]) <= bound).all()
    matrix = PW.gene_pathway_matrix(g["gene_sets"])
    assert list(matrix.index) == [str(v) for v in g["matrix_genes"]] and list(matrix.columns) == [str(v) for v in g["matrix_names"]]
    assert np.array_equal(matrix.values, g["matrix"])
    # a frame whose columns come in another order scores the same
    shuffled = expression[list(reversed(columns))]
    assert np.array_equal(s.score(shuffled).values, got.values)


# ---- 5. the planted consistency design --------------------------------------------------------------------------------------------
def _consistency(c, block, real_block=None, method="mean", comm=None):
    from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
    return PW.pathway_consistency(comm or ShardComm(False), NumpyKernels(), "cpu", c["synth"], block, c["sets"], c["real"], real_block,
                                  method=method)


@pytest.mark.parametrize("method", ["mean", "ssgsea"])
def test_planted_consistency_tells_faithful_from_decoupled(method):
    from osteosarcoma_diffusionmodel_amd.validation import marginal_ks
    from marginal_helpers import marginals64
    c = planted_cohorts(method)
    faithful, rows = _consistency(c, c["faithful"], c["real_block"], method)
    decoupled, drows = _consistency(c, c["decoupled"], None, method)
    print(method, {k: v for k, v in faithful.items()}, {k: v for k, v in decoupled.items()})
    assert faithful["pwc_pearson_min"] >= 0.98 and faithful["pwc_rmse_max"] <= 0.15
    assert np.nanmax(np.abs(drows["synthetic"]["pearson"])) <= 5 / np.sqrt(N_SYNTH) and decoupled["pwc_rmse_mean"] >= 1.0
    assert faithful["pwc_r2"] > 0.97 and decoupled["pwc_r2"] < 0.0
    assert faithful["pwc_pathways"] == 7 and faithful["pwc_pathways_skipped"] == 0 and faithful["pwc_constant"] == 0
    assert faithful["pwc_rows_nonfinite"] == 0 and faithful["pwc_pearson_min_pathway"] in c["names"]
    assert faithful["pwc_rmse_max_pathway"] in c["names"]
    # the real cohort's own block: r = 1 and rmse = 0 up to its fp32 rounding
    assert faithful["pwc_real_pearson_min"] >= 1 - 1e-9 and faithful["pwc_real_rmse_max"] <= 1e-6
    assert not any(k.startswith("pwc_real_") for k in decoupled)
    # every marginal of the pathway columns is the same in both cohorts: that is the point of the check
    ks = [marginal_ks({**marginals64(c["real_block"], b), "n1": len(c["real_block"]), "n2": len(b)}) for b in (c["faithful"], c["decoupled"])]
    assert np.array_equal(ks[0], ks[1])
    # per-pathway definitions, restated
    z, g = c["z"], c["faithful"].astype(np.float64)
    want_r = [np.corrcoef(g[:, q], z[:, q])[0, 1] for q in range(7)]
    assert np.allclose(rows["synthetic"]["pearson"], want_r, rtol=0, atol=1e-12)
    assert np.allclose(rows["synthetic"]["rmse"], np.sqrt(((g - z) ** 2).mean(axis=0)), rtol=1e-12)
    assert np.allclose(rows["synthetic"]["bias"], g.mean(axis=0) - z.mean(axis=0), rtol=0, atol=1e-13)
    assert np.allclose(rows["synthetic"]["sd_ratio"], g.std(axis=0) / z.std(axis=0), rtol=1e-11)
    assert np.isclose(faithful["pwc_r2"], 1 - ((g - z) ** 2).sum() / ((z - z.mean(axis=0)) ** 2).sum(), rtol=1e-11)


def test_consistency_counts_nonfinite_rows_and_constant_pathways():
    c = planted_cohorts("mean")
    block = c["faithful"].copy()
    block[3, 2], block[10, 2], block[11, 5] = np.nan, np.inf, np.nan
    block[:, 6] = 1.5                                                             # a constant pathway column: no r
    summary, rows = _consistency(c, block)
    assert summary["pwc_rows_nonfinite"] == 3 and rows["synthetic"]["n"].tolist() == [900, 900, 898, 900, 900, 899, 900]
    assert summary["pwc_constant"] == 1 and np.isnan(rows["synthetic"]["pearson"][6]) and np.isfinite(summary["pwc_pearson_min"])
    frames = _consistency({**c, "synth": pd.DataFrame(c["synth"], columns=[f"g{i}" for i in range(N_GENES)]),
                           "real": pd.DataFrame(c["real"], columns=[f"g{i}" for i in range(N_GENES)])},
                          pd.DataFrame(c["faithful"][:, ::-1], columns=c["names"][::-1]))[0]
    assert frames == _consistency(c, c["faithful"])[0]                            # frames are matched by name


# ---- 6. sharded over gloo ---------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from osteosarcoma_diffusionmodel_amd.parallel import ShardComm, shard_rows
        c = planted_cohorts("mean")
        off, cnt = shard_rows(N_SYNTH, rank, world)
        local = {**c, "synth": c["synth"][off:off + cnt]}
        comm = ShardComm(True)
        assert comm.on and comm.world == world
        got = _consistency(local, c["faithful"][off:off + cnt], c["real_block"], comm=comm)[0]
        ref = _consistency(c, c["faithful"], c["real_block"])[0]
        ok = list(got) == list(ref)
        for key, v in ref.items():
            ok &= got[key] == v if isinstance(v, (str, int)) else bool(np.isclose(got[key], v, rtol=1e-12, atol=1e-13))
        q.put((rank, bool(ok)))
    except Exception as e:                           # report instead of leaving the parent to time out
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_sharded_consistency_equals_single_process_gloo():
    world = 3
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(r, True) for r in range(world)]


# ---- 7. fit, state, config and arguments ------------------------------------------------------------------------------------------
def test_fit_standardisation_and_state_round_trip():
    c = planted_cohorts("mean")
    for method in ("mean", "zscore", "ssgsea"):
        s = scorer(c["sets"], list(range(N_GENES)), method=method)
        if method == "zscore":
            with pytest.raises(ValueError, match="fit"):
                s.score(c["real"])
        with pytest.raises(ValueError, match="fit"):
            s.score(c["real"], standardize=True)
        s.fit(c["real"])
        p = s.score(c["real"]).numpy()
        frame = pd.DataFrame(p)
        want = ((frame - frame.mean()) / (frame.std() + 1e-8)).values              # what prepare_data does to pathway_scores.csv
        assert np.allclose(s.score(c["real"], standardize=True).numpy(), want, rtol=1e-12, atol=1e-12)
        if method == "zscore":
            x = c["real"].astype(np.float64)
            assert np.allclose(s.center, x.mean(axis=0), rtol=1e-6) and np.allclose(s.scale, 1 / x.std(axis=0, ddof=1), rtol=1e-6)
            z = ((x - s.center.astype(np.float64)) * s.scale.astype(np.float64))
            assert np.allclose(p[:, 3], z[:, c["sets"]["SET_30"]].sum(axis=1) / np.sqrt(30), rtol=1e-12, atol=1e-12)
        state = s.state()
        assert all(isinstance(v, np.ndarray) for v in state.values())
        back = PW.PathwayScorer.from_state({k: v.copy() for k, v in state.items()}, device="cpu", kernels=NumpyKernels())
        assert back.names == s.names and back.genes == s.genes and back.method == method and back.skipped == s.skipped
        assert np.array_equal(back.score(c["synth"], standardize=True).numpy(), s.score(c["synth"], standardize=True).numpy())
    const = scorer(c["sets"], list(range(N_GENES)), method="zscore").fit(np.where(np.arange(N_GENES) == 4, 2.0, c["real"]))
    assert const.scale[4] == 0.0 and np.isfinite(const.score(c["synth"]).numpy()).all()


def _write_cohort(tmp_path, with_scores):
    rs = np.random.default_rng(3)
    genes = [f"G{i}" for i in range(20)]
    patients = [f"p{i}" for i in range(12)]
    expr = pd.DataFrame(rs.gamma(2.0, 1.5, (12, 20)).astype(np.float32), index=patients, columns=genes)
    mut = pd.DataFrame((rs.random((12, 8)) < 0.4).astype(np.float32), index=patients, columns=genes[:8])
    clin = pd.DataFrame({"submitter_id": patients, "survival_days": rs.integers(10, 900, 12).astype(float), "event_occurred": 1.0,
                         "age_years": rs.integers(5, 30, 12).astype(float)})
    expr.to_csv(tmp_path / "expression_matrix_aligned.csv")
    mut.to_csv(tmp_path / "mutation_matrix_aligned.csv")
    clin.to_csv(tmp_path / "clinical_aligned.csv", index=False)
    sets = {"A": genes[:6], "B": genes[4:16], "TOO_THIN": genes[:3] + ["ZZ1", "ZZ2"], "C": genes[10:] + ["ZZ3"]}
    PW.write_gmt(sets, tmp_path / "sets.gmt")
    if with_scores:
        pd.DataFrame(rs.standard_normal((12, 2)), index=patients, columns=["X", "Y"]).to_csv(tmp_path / "pathway_scores.csv")
    return expr, mut, sets


def test_prepare_data_computes_missing_pathway_scores_from_the_gene_sets_file(tmp_path, monkeypatch):
    from osteosarcoma_diffusionmodel_amd.train import prepare_data
    expr, mut, sets = _write_cohort(tmp_path, with_scores=False)
    conf = {"data": {"processed_dir": str(tmp_path)}, "model": {}, "training": {"val_split": 0.0, "random_seed": 1, "batch_size": 2}}
    with pytest.raises(FileNotFoundError, match="pathway_features.py"):          # without the key: today's error
        prepare_data(conf)
    assert not (tmp_path / "pathway_scores.csv").exists()
    conf["data"]["gene_sets_file"] = str(tmp_path / "sets.gmt")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):                # the scores are a device computation
            prepare_data(conf)
    monkeypatch.setattr(PW, "_device_kernels", lambda device: NumpyKernels())
    _, _, conf = prepare_data(conf)
    assert conf["model"]["n_pathways"] == 3 and conf["model"]["n_genes_expression"] == 20
    scores = pd.read_csv(tmp_path / "pathway_scores.csv", index_col=0)
    assert list(scores.columns) == ["A", "B", "C"] and list(scores.index) == list(expr.index)
    assert np.allclose(scores["B"].values, expr[sets["B"]].astype(np.float64).mean(axis=1).values, rtol=1e-12)
    burden = pd.read_csv(tmp_path / "pathway_mutation_scores.csv", index_col=0)
    assert list(burden.columns) == ["A"] and np.allclose(burden["A"].values, mut[sets["A"]].sum(axis=1).values / 6)
    matrix = pd.read_csv(tmp_path / "gene_pathway_matrix.csv", index_col=0)
    assert list(matrix.columns) == list(sets) and matrix.values.sum() == sum(len(v) for v in sets.values())
    conf["data"]["pathway_scoring"] = "ssgsea"
    (tmp_path / "pathway_scores.csv").unlink()
    prepare_data(conf)
    x = expr.values.astype(np.float32)
    cols = [[list(expr.columns).index(g) for g in sets[n] if g in expr.columns] for n in ("A", "B", "C")]
    assert np.allclose(pd.read_csv(tmp_path / "pathway_scores.csv", index_col=0).values, ssgsea64(x, cols, rank_table(20)), rtol=1e-12)


def test_prepare_data_leaves_an_existing_scores_file_alone(tmp_path, monkeypatch):
    from osteosarcoma_diffusionmodel_amd.train import prepare_data
    _write_cohort(tmp_path, with_scores=True)
    before = (tmp_path / "pathway_scores.csv").read_bytes()
    monkeypatch.setattr(PW, "compute_pathway_features", lambda *a, **k: pytest.fail("must not be called"))
    conf = {"data": {"processed_dir": str(tmp_path), "gene_sets_file": str(tmp_path / "sets.gmt")}, "model": {},
            "training": {"val_split": 0.0, "random_seed": 1, "batch_size": 2}}
    _, _, conf = prepare_data(conf)
    assert conf["model"]["n_pathways"] == 2 and (tmp_path / "pathway_scores.csv").read_bytes() == before


def _prepare_worker(rank, world, port, root, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pathlib import Path
        from osteosarcoma_diffusionmodel_amd.train import prepare_data
        calls = []
        real = PW.compute_pathway_features

        def counted(config, **kw):
            calls.append(rank)
            return real(config, **kw)

        PW._device_kernels = lambda device: NumpyKernels()
        PW.compute_pathway_features = counted
        conf = {"data": {"processed_dir": root, "gene_sets_file": str(Path(root) / "sets.gmt")}, "model": {},
                "training": {"val_split": 0.25, "random_seed": 1, "batch_size": 2}}
        train_loader, _, conf = prepare_data(conf)
        scores = pd.read_csv(Path(root) / "pathway_scores.csv", index_col=0)
        leftovers = [p.name for p in Path(root).iterdir() if p.name.endswith(".part")]
        first = (len(calls), conf["model"]["n_pathways"], len(train_loader.sampler), tuple(scores.shape), leftovers)
        prepare_data(conf)                               # the file is there now: nobody computes
        bad = dict(conf, data=dict(conf["data"], processed_dir=root + "/bad"))
        try:                                             # rank 0's error reaches every rank instead of leaving them waiting
            prepare_data(bad)
            failed = "no error"
        except RuntimeError as e:
            failed = "rank 0" in str(e)
        q.put((rank, first, len(calls), failed))
    except Exception as e:                           # report instead of leaving the parent to time out
        q.put((rank, repr(e), None, None))
        raise
    finally:
        dist.destroy_process_group()


def test_prepare_data_computes_the_scores_once_under_data_parallel_gloo_world2(tmp_path):
    """Two ranks, ``gene_sets_file`` set and no scores file: rank 0 alone computes, both read the whole file and draw equal shards; a
    failure on rank 0 (here: a scores-less directory whose expression CSV holds a gene too few for any set) is raised on both."""
    expr, _, _ = _write_cohort(tmp_path, with_scores=False)
    bad = tmp_path / "bad"
    bad.mkdir()
    for name in ("mutation_matrix_aligned.csv", "clinical_aligned.csv"):
        (bad / name).write_bytes((tmp_path / name).read_bytes())
    expr.iloc[:, :2].to_csv(bad / "expression_matrix_aligned.csv")      # two genes: no set is left, the scorer raises
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_prepare_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res[0] == (0, (1, 3, 4, (12, 3), []), 2, True), res              # one call that wrote the files, none for the second
    assert res[1] == (1, (0, 3, 4, (12, 3), []), 0, True), res              # prepare_data, one that failed in the other directory


def test_argument_errors_and_signatures():
    from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels
    c = planted_cohorts("mean")
    with pytest.raises(ValueError, match="fit"):
        scorer(c["sets"], list(range(N_GENES)), method="zscore").score(c["real"])
    with pytest.raises(ValueError, match="genes"):                                # mismatched widths
        _consistency({**c, "synth": c["synth"][:, :80]}, c["faithful"])
    with pytest.raises(ValueError, match="narrower"):                             # a block narrower than the kept sets
        _consistency(c, c["faithful"][:, :6])
    with pytest.raises(ValueError, match="wider"):
        _consistency(c, np.concatenate([c["faithful"], c["faithful"][:, :1]], axis=1))
    with pytest.raises(ValueError, match="rows"):
        _consistency(c, c["faithful"][:-1])
    with pytest.raises(ValueError, match="lacks"):
        _consistency(c, pd.DataFrame(c["faithful"], columns=["nope"] + c["names"][1:]))
    with pytest.raises(ValueError, match="expression matrix"):
        scorer(c["sets"], list(range(N_GENES))).score(c["real"][:, :50])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PW.PathwayScorer(c["sets"], list(range(N_GENES)), device="cpu")                # no kernels given, no ROCm device named
    v = inspect.signature(BiologicalValidator.validate_all).parameters
    assert v["consistency"].default is False and v["consistency_method"].default == "mean"
    p = inspect.signature(BiologicalValidator.pathway_consistency).parameters
    assert list(p)[1:9] == ["synth_expression", "synth_pathways", "gene_sets", "real_expression", "real_pathways", "method", "alpha",
                            "return_rows"]
    assert p["real_pathways"].default is None and p["method"].default == "mean" and p["alpha"].default == 0.25
    assert "sharded" in BiologicalValidator.pathway_consistency.__doc__
    for name in ("pathway_scores", "pathway_agreement"):                          # the stand-in takes what the device kernels take
        assert list(inspect.signature(getattr(DeviceKernels, name)).parameters)[1:] == list(inspect.signature(getattr(NumpyKernels, name)).parameters)
