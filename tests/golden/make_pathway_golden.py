"""Makes tests/golden/g11_pathway_scores.npz from a checkout of the reference project:

    python tests/golden/make_pathway_golden.py /path/to/Osteosarcoma_DiffusionModel

Runs the three methods of the reference's utils/pathway_features.py (``compute_pathway_scores_from_expression``,
``compute_pathway_scores_from_mutations``, ``create_gene_pathway_matrix``) on a 40 x 300 random frame whose columns are 250 of the
reference's own gene symbols plus 50 that are in no set (two sets keep fewer than five genes and drop out), and stores the inputs,
the outputs, the column names and the set lists.  The fixture is the only place the reference's curated sets appear in this
repository (tests/test_pathways_cpu.py reads them back).
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import pandas as pd

ROWS, KEPT, OTHERS, SEED = 40, 250, 50, 11
DROPPED = (10, 28)                                      # two sets the frame is too narrow for


def load_reference(root):
    if "requests" not in sys.modules:                      # imported at the module's top, never used by the three methods
        try:
            import requests  # noqa: F401
        except ImportError:
            sys.modules["requests"] = types.ModuleType("requests")
    spec = importlib.util.spec_from_file_location("reference_pathway_features", Path(root) / "utils" / "pathway_features.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PathwayFeatureEngineering(pathway_database="hallmark")


def main(root):
    eng = load_reference(root)
    gene_sets = eng.load_gene_sets()
    names = list(gene_sets)
    thinned = {names[i] for i in DROPPED}                  # their own genes stay out of the columns: fewer than 5 are left
    own = {g for n in thinned for g in gene_sets[n]} - {g for n in names if n not in thinned for g in gene_sets[n]}
    symbols = sorted({g for members in gene_sets.values() for g in members} - own)
    rs = np.random.default_rng(SEED)
    columns = list(rs.permutation(symbols)[:KEPT]) + [f"OTHER{i}" for i in range(OTHERS)]
    columns = [str(c) for c in rs.permutation(columns)]
    patients = [f"P{i:03d}" for i in range(ROWS)]
    values = np.where(rs.random((ROWS, len(columns))) < 0.3, 0.0, rs.gamma(2.0, 1.5, (ROWS, len(columns)))).astype(np.float32)
    expression = pd.DataFrame(values.astype(np.float64), index=patients, columns=columns)
    mutations = pd.DataFrame((rs.random((ROWS, len(columns))) < 0.2).astype(np.float64), index=patients, columns=columns)
    scores = eng.compute_pathway_scores_from_expression(expression)
    burden = eng.compute_pathway_scores_from_mutations(mutations)
    matrix = eng.create_gene_pathway_matrix()
    out = Path(__file__).resolve().parent / "g11_pathway_scores.npz"
    np.savez_compressed(
        out, columns=np.array(columns), patients=np.array(patients), expression=values, mutations=mutations.values.astype(np.float32),
        set_names=np.array(names), set_offsets=np.cumsum([0] + [len(gene_sets[n]) for n in names]).astype(np.int64),
        set_members=np.array([g for n in names for g in gene_sets[n]]),
        score_names=np.array([str(c) for c in scores.columns]), scores=scores.values.astype(np.float64),
        burden_names=np.array([str(c) for c in burden.columns]), burden=burden.values.astype(np.float64),
        matrix_genes=np.array([str(g) for g in matrix.index]), matrix_names=np.array([str(c) for c in matrix.columns]),
        matrix=matrix.values.astype(np.int8))
    print(f"{out}: {out.stat().st_size} bytes, {scores.shape[1]} of {len(names)} sets scored")


if __name__ == "__main__":
    main(sys.argv[1])
