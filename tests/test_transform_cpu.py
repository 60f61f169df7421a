"""CPU: the host half of the feature transforms (transform.py) -- the fit against NumPy's quantiles and the
float64 restatement of tests/transform_helpers.py, checkpoint transport, ``map_bounds``, every ValueError that needs no device, and
the argument checks of ``osd_xf_apply`` that return before any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import transform as XF
from osteosarcoma_diffusionmodel_amd.transform import FeatureTransform
from transform_helpers import bits, ref_forward, ref_knots, ref_levels

BLOCKS = {"mutations": 3, "expression": 5, "pathways": 2}
SPEC = {"expression": "quantile_normal", "pathways": "standard"}


def _features(n, seed=0, blocks=BLOCKS):
    rs = np.random.default_rng(seed)
    md, ed, pd_ = blocks["mutations"], blocks["expression"], blocks["pathways"]
    x = np.concatenate([rs.integers(0, 2, (n, md)).astype(np.float32), np.exp(rs.normal(1, 1, (n, ed))).astype(np.float32),
                        rs.normal(2, 3, (n, pd_)).astype(np.float32)], axis=1)
    return x


def _ulp_apart(a, b):
    """|a - b| in units of the float32 spacing at max(|a|, |b|)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


# ---- fit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, nq", [(50, 1000), (200, 100), (1500, 1000), (1030, 2000), (7, 3), (9, 2)])
def test_knots_are_numpys_linear_quantiles(n, nq):
    x = _features(n, seed=n)
    ft = FeatureTransform.fit(x, BLOCKS, SPEC, n_quantiles=nq)
    Q = min(nq, n, 1024)
    assert tuple(ft.knots.shape) == (10, Q) and tuple(ft.levels.shape) == (Q,)
    knots = ft.knots.numpy()
    for f in range(3, 8):
        col64 = x[:, f].astype(np.float64)
        want = np.quantile(col64, np.arange(Q) / (Q - 1), method="linear").astype(np.float32)
        assert _ulp_apart(knots[f], want).max() <= 1.0
        assert (bits(knots[f]) == bits(ref_knots(x[:, f], Q))).all()        # the restatement: quotient and remainder in integers
    assert (knots[:3] == 0).all() and (knots[8:] == 0).all()
    assert ft.kind.tolist() == [0, 0, 0, 2, 2, 2, 2, 2, 1, 1]


def test_knots_are_the_sorted_column_when_Q_is_n():
    x = _features(321, seed=3)
    ft = FeatureTransform.fit(x, BLOCKS, SPEC, n_quantiles=321)
    for f in range(3, 8):
        assert (bits(ft.knots.numpy()[f]) == bits(np.sort(x[:, f]))).all()


@pytest.mark.parametrize("Q", [2, 3, 100, 1000, 1024])
def test_knots_non_decreasing_and_levels_strictly_increasing(Q):
    x = _features(1100, seed=Q)
    x[:, 4] = np.round(x[:, 4])                                     # ties
    ft = FeatureTransform.fit(x, BLOCKS, SPEC, n_quantiles=Q)
    knots, levels = ft.knots.numpy(), ft.levels.numpy()
    assert knots.shape[1] == Q and (np.diff(knots, axis=1) >= 0).all()
    assert levels.dtype == np.float32 and (np.diff(levels) > 0).all()
    assert (levels == -levels[::-1]).all()                          # antisymmetric, exactly: the middle of an odd table is 0
    assert _ulp_apart(levels, ref_levels(Q)).max() <= 1.0           # another Phi^-1
    assert abs(float(levels[0]) + 5.199337582) < 1e-5               # Phi^-1(1e-7)


def test_n_quantiles_above_1024_is_capped():
    ft = FeatureTransform.fit(_features(1500), BLOCKS, SPEC, n_quantiles=5000)
    assert ft.levels.shape[0] == 1024 and ft.n_quantiles == 5000


def test_nan_entries_are_ignored_per_column():
    x = _features(300, seed=11)
    holes = np.random.default_rng(1).random(x.shape) < 0.2
    holes[:, 3] = False
    xn = np.where(holes, np.nan, x).astype(np.float32)
    xn[5, 9] = np.inf                                               # not finite: ignored like NaN
    ft = FeatureTransform.fit(xn, BLOCKS, SPEC, n_quantiles=1000)
    Q = int(np.isfinite(xn[:, 3:8]).sum(0).min())                   # the fewest finite rows of a quantile column
    assert ft.levels.shape[0] == Q
    for f in range(3, 8):
        assert (bits(ft.knots.numpy()[f]) == bits(ref_knots(xn[:, f], Q))).all()
    for f in (8, 9):
        col = xn[:, f].astype(np.float64)
        col = col[np.isfinite(col)]
        assert ft.center[f].item() == np.float32(col.mean())
        assert ft.scale[f].item() == np.float32(col.std(ddof=1) + 1e-8)


def test_constant_column_maps_to_zero():
    x = _features(100, seed=2)
    x[:, 5] = 3.25
    for Q in (100, 33):
        ft = FeatureTransform.fit(x, BLOCKS, SPEC, n_quantiles=Q)
        assert (ft.knots.numpy()[5] == np.float32(3.25)).all()
        v = np.zeros(10, dtype=np.float32)
        v[5] = 3.25
        assert ft.forward_host(v)[5] == 0.0                         # the mid-rank level of the whole table
    x[:, 9] = -1.5                                                  # a constant standard column: scale is the 1e-8 floor
    ft = FeatureTransform.fit(x, BLOCKS, SPEC)
    assert ft.center[9].item() == -1.5 and ft.scale[9].item() == np.float32(1e-8)


def test_zero_inflated_column_has_a_plateau_of_the_right_length():
    n = 1000
    x = _features(n, seed=4)
    x[:300, 6] = 0.0                                                # 30 % zeros, the rest positive
    ft = FeatureTransform.fit(x, BLOCKS, SPEC, n_quantiles=1000)
    k, zl = ft.knots.numpy()[6], ft.levels.numpy()
    assert int((k == 0).sum()) == 300 and (k[:300] == 0).all() and k[300] > 0
    v = np.zeros(10, dtype=np.float32)
    z0 = ft.forward_host(v)[6]
    assert z0 == np.float32(0.5) * (zl[149] + zl[150])              # the mid-rank level: Phi^-1 of about 0.15, not a -5.2 tail mean
    assert abs(float(z0) + 1.0364) < 0.01


def test_forward_host_is_the_rule():
    """``forward_host`` (what ``map_bounds`` evaluates) against the float64 restatement, one value per column."""
    x = _features(400, seed=6)
    x[:100, 7] = 0.0
    ft = FeatureTransform.fit(x, BLOCKS, SPEC, n_quantiles=200)
    t = (ft.kind.numpy(), ft.knots.numpy(), ft.levels.numpy(), ft.center.numpy(), ft.scale.numpy())
    rs = np.random.default_rng(0)
    for trial in range(20):
        v = x[rs.integers(0, 400)].copy() if trial % 2 else (x[rs.integers(0, 400)] * rs.uniform(0.5, 1.5, 10)).astype(np.float32)
        ref, exact, tol = ref_forward(v[None, :], *t)
        got = ft.forward_host(v)
        assert (bits(got)[exact[0]] == bits(ref[0].astype(np.float32))[exact[0]]).all()
        assert (np.abs(got.astype(np.float64) - ref[0])[~exact[0]] <= tol[0][~exact[0]]).all()


# ---- transport ----------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_weights_only(tmp_path):
    ft = FeatureTransform.fit(_features(150), BLOCKS, SPEC, n_quantiles=64)
    torch.save({"feature_transform": ft.state_dict()}, tmp_path / "t.pt")
    back = FeatureTransform.from_state_dict(torch.load(tmp_path / "t.pt", map_location="cpu", weights_only=True)["feature_transform"])
    for name in ("kind", "knots", "levels", "center", "scale"):
        a, b = getattr(ft, name), getattr(back, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert back.blocks == ft.blocks == BLOCKS and back.spec == ft.spec and back.n_quantiles == 64
    assert back.spec == {"mutations": "identity", "expression": "quantile_normal", "pathways": "standard"}
    sd = ft.state_dict()
    assert all(isinstance(sd[k], torch.Tensor) for k in ("kind", "knots", "levels", "center", "scale"))
    with pytest.raises(ValueError, match="lacks"):
        FeatureTransform.from_state_dict({k: v for k, v in sd.items() if k != "knots"})
    sd["levels"] = sd["levels"].flip(0)
    with pytest.raises(ValueError, match="strictly increasing"):
        FeatureTransform.from_state_dict(sd)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def test_map_bounds_is_monotone_and_keeps_infinities():
    x = _features(500, seed=8)
    x[:150, 3] = 0.0
    ft = FeatureTransform.fit(x, BLOCKS, SPEC, n_quantiles=100)
    rs = np.random.default_rng(2)
    lo = np.full(10, -np.inf, dtype=np.float32)
    hi = np.full(10, np.inf, dtype=np.float32)
    lo[:3], hi[:3] = 0.0, 1.0
    lo[3:8], hi[3:6] = 0.0, [2.0, 5.0, 1e9]
    lo[8], hi[8] = -1.0, 4.0
    mlo, mhi = ft.map_bounds(lo, hi)
    assert mlo.dtype == mhi.dtype == np.float32
    assert (mlo[:3] == 0).all() and (mhi[:3] == 1).all()            # identity
    assert np.isposinf(mhi[6:8]).all() and np.isposinf(mhi[9]) and np.isneginf(mlo[9])
    assert (mlo <= mhi).all()
    zl = ft.levels.numpy()
    assert mhi[5] == zl[-1]                                         # above every knot
    assert mlo[3] == np.float32(0.5) * (zl[14] + zl[15])            # 0 sits on the zero plateau (knots 0..29 of 100): its mid-rank level
    assert mlo[8] == (np.float32(-1.0) - ft.center.numpy()[8]) / ft.scale.numpy()[8]          # fp32 arithmetic
    # monotone: ascending data values never map to descending model values
    for f in range(3, 10):
        grid = np.sort(rs.uniform(x[:, f].min() - 1, x[:, f].max() + 1, 64).astype(np.float32))
        mapped = []
        for g in grid:
            v = np.zeros(10, dtype=np.float32)
            v[f] = g
            mapped.append(ft.map_bounds(v, v)[0][f])
        assert (np.diff(np.array(mapped, dtype=np.float64)) >= 0).all()
    with pytest.raises(ValueError, match="NaN"):
        ft.map_bounds(np.full(10, np.nan, dtype=np.float32), hi)
    with pytest.raises(ValueError, match="expected"):
        ft.map_bounds(lo[:5], hi[:5])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_fit_value_errors():
    x = _features(40)
    with pytest.raises(ValueError, match="mutations must stay identity"):
        FeatureTransform.fit(x, BLOCKS, {"mutations": "standard"})
    with pytest.raises(ValueError, match="unknown block"):
        FeatureTransform.fit(x, BLOCKS, {"methylation": "standard"})
    with pytest.raises(ValueError, match="unknown kind"):
        FeatureTransform.fit(x, BLOCKS, {"expression": "yeo_johnson"})
    with pytest.raises(ValueError, match="n_quantiles"):
        FeatureTransform.fit(x, BLOCKS, SPEC, n_quantiles=1)
    bad = x.copy()
    bad[:, 4] = np.nan
    with pytest.raises(ValueError, match="column 4 has no finite value"):
        FeatureTransform.fit(bad, BLOCKS, SPEC)
    bad[:, 4] = x[:, 4]
    bad[:, 1] = np.nan                                              # an identity column needs no fit
    FeatureTransform.fit(bad, BLOCKS, SPEC)
    with pytest.raises(ValueError, match="expected"):
        FeatureTransform.fit(x[:, :9], BLOCKS, SPEC)
    assert FeatureTransform.fit(torch.from_numpy(x), BLOCKS, {}).kind.tolist() == [0] * 10      # a missing block is identity


def test_transform_config():
    assert XF.transform_config({}) is None and XF.transform_config({"data": {}}) is None and XF.transform_config({"data": {"transform": None}}) is None
    spec, nq = XF.transform_config({"data": {"transform": {"expression": "quantile_normal", "pathways": "standard", "n_quantiles": 1000}}})
    assert spec == {"mutations": "identity", "expression": "quantile_normal", "pathways": "standard"} and nq == 1000
    assert XF.transform_config({"data": {"transform": {"expression": "standard"}}})[1] is None
    for bad in ({"n_quantiles": 1}, {"mutations": "quantile_normal"}, {"expression": "log"}, {"genes": "standard"}, "quantile_normal"):
        with pytest.raises(ValueError, match="data.transform"):
            XF.transform_config({"data": {"transform": bad}})


def test_checkpoint_spec_mismatch_raises():
    """The ``checkpoint_prediction_type`` rule for ``data.transform``: absent adopts, equal passes, different raises."""
    ft = FeatureTransform.fit(_features(80), BLOCKS, SPEC, n_quantiles=50)
    ckpt = {"feature_transform": ft.state_dict()}
    got = XF.checkpoint_feature_transform(ckpt, {"data": {}})
    assert got.spec == ft.spec and torch.equal(got.knots, ft.knots)
    same = {"data": {"transform": {"expression": "quantile_normal", "pathways": "standard", "n_quantiles": 50}}}
    assert torch.equal(XF.checkpoint_feature_transform(ckpt, same).levels, ft.levels)
    assert XF.checkpoint_feature_transform(ckpt, {"data": {"transform": dict(SPEC)}}) is not None       # n_quantiles not named: the checkpoint's
    with pytest.raises(ValueError, match=r"data.*transform.*checkpoint was trained with"):
        XF.checkpoint_feature_transform(ckpt, {"data": {"transform": {"expression": "standard", "pathways": "standard"}}})
    with pytest.raises(ValueError, match="n_quantiles=64"):
        XF.checkpoint_feature_transform(ckpt, {"data": {"transform": dict(SPEC, n_quantiles=64)}})
    with pytest.raises(ValueError, match="trained without data.transform"):
        XF.checkpoint_feature_transform({}, {"data": {"transform": dict(SPEC)}})
    assert XF.checkpoint_feature_transform({}, {"data": {}}) is None
    assert XF.checkpoint_feature_transform({}, {"data": {"transform": {"expression": "identity"}}}) is None


def test_load_trained_model_refuses_another_spec(tmp_path):
    import pandas as pd
    from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, load_trained_model
    conf = {"data": {"processed_dir": str(tmp_path)},
            "model": {"architecture": "diffusion", "latent_dim": 128, "hidden_dims": [32, 64, 32], "gnn": {"dropout": 0.0},
                      "diffusion": {"num_steps": 10, "beta_schedule": "cosine"}}}
    for fname, w in (("mutation_matrix_aligned.csv", 3), ("expression_matrix_aligned.csv", 5), ("pathway_scores.csv", 2)):
        pd.DataFrame(np.zeros((1, w)), index=["r0"], columns=[f"c{i}" for i in range(w)]).to_csv(tmp_path / fname)
    model = BiologyAwareDiffusionModel(3, 5, 2, 4, conf)
    ft = FeatureTransform.fit(_features(60), BLOCKS, SPEC, n_quantiles=32)
    torch.save({"model_state_dict": model.state_dict(), "config": conf, "feature_transform": ft.state_dict()}, tmp_path / "c.pt")
    loaded = load_trained_model(tmp_path / "c.pt", conf, "cpu")
    assert loaded.feature_transform.spec == ft.spec and torch.equal(loaded.feature_transform.knots, ft.knots)
    other = {**conf, "data": {**conf["data"], "transform": {"expression": "standard"}}}
    with pytest.raises(ValueError, match="data.*transform"):
        load_trained_model(tmp_path / "c.pt", other, "cpu")
    torch.save({"model_state_dict": model.state_dict(), "config": conf}, tmp_path / "plain.pt")
    assert load_trained_model(tmp_path / "plain.pt", conf, "cpu").feature_transform is None
    with pytest.raises(ValueError, match="trained without data.transform"):
        load_trained_model(tmp_path / "plain.pt", other, "cpu")
    with pytest.raises(ValueError, match="cVAE"):
        load_trained_model(tmp_path / "c.pt", {**conf, "model": {**conf["model"], "architecture": "cvae"}}, "cpu")


def test_training_refusals_name_data_transform():
    from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel

    class Vae:
        vae = object()

    with pytest.raises(ValueError, match="data.transform.*cVAE"):
        XF.check_transform_training(Vae(), False)
    with pytest.raises(ValueError, match="data.transform.*constraint losses"):
        XF.check_transform_training(object(), True)
    XF.check_transform_training(object(), False)
    conf = {"model": {"latent_dim": 128, "hidden_dims": [32, 64, 32], "gnn": {"dropout": 0.0},
                      "diffusion": {"num_steps": 10, "beta_schedule": "cosine"}}}
    model = BiologyAwareDiffusionModel(3, 5, 2, 4, conf)
    assert model.feature_transform is None
    model.feature_transform = FeatureTransform.fit(_features(60), BLOCKS, SPEC, n_quantiles=32)
    with pytest.raises(ValueError, match="data.transform"):
        model.set_constraints(pathways=[[3, 4, 5]])
    model.set_constraints(pathways=[[3, 4, 5]], pathway_weight=0.0, mutexpr_weight=0.0)       # switched off: nothing to refuse
    model.set_constraints()


def test_model_and_dataset_transforms_must_agree():
    """``training_transform``, the Trainer's rule: the dataset's map, else the model's own; a model whose map differs from the dataset's,
    or that meets an untransformed dataset, is a ValueError naming ``data.transform``."""
    a = FeatureTransform.fit(_features(60, seed=1), BLOCKS, SPEC, n_quantiles=32)
    same = FeatureTransform.from_state_dict(a.state_dict())
    other_rows = FeatureTransform.fit(_features(60, seed=2), BLOCKS, SPEC, n_quantiles=32)
    other_spec = FeatureTransform.fit(_features(60, seed=1), BLOCKS, {"expression": "standard", "pathways": "standard"}, n_quantiles=32)
    assert a.same_as(same) and not a.same_as(other_rows) and not a.same_as(other_spec)
    assert XF.training_transform(None, None, True) is None and XF.training_transform(None, None, False) is None
    assert XF.training_transform(None, a, False) is a                    # a fresh model adopts the dataset's
    assert XF.training_transform(same, a, False) is a                    # a loaded model on data prepared the same way
    assert XF.training_transform(a, None, False) is a                    # a loader the Trainer cannot look into: the model's own
    for other in (other_rows, other_spec):
        with pytest.raises(ValueError, match="data.transform"):
            XF.training_transform(other, a, False)
    with pytest.raises(ValueError, match="prepared without data.transform"):
        XF.training_transform(a, None, True)


def test_prepare_data_refuses_a_cvae(tmp_path):
    from osteosarcoma_diffusionmodel_amd.train import prepare_data
    from transform_helpers import tiny_config, write_cohort
    write_cohort(tmp_path, n=20)
    conf = tiny_config(tmp_path, tmp_path / "ckpt", {"expression": "quantile_normal"})
    conf["model"]["architecture"] = "cvae"
    with pytest.raises(ValueError, match="data.transform.*cVAE"):
        prepare_data(conf)
    conf["model"]["architecture"] = "diffusion"
    conf["data"]["transform"] = {"mutations": "standard"}
    with pytest.raises(ValueError, match="mutations must stay identity"):
        prepare_data(conf)


# ---- no CPU fallback ----------------------------------------------------------------------------------------------------------------
def test_forward_on_a_cpu_tensor_raises():
    ft = FeatureTransform.fit(_features(60), BLOCKS, SPEC, n_quantiles=32)
    x = torch.zeros(4, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.forward(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.inverse(x, out=x)
    with pytest.raises(ValueError, match="expected a"):
        ft.forward(torch.zeros(4, 9))


def test_xf_apply_rejects_bad_arguments_on_the_host():
    """Every OSD_EINVAL of osd_xf_apply that the host can see is returned before any device call; rows == 0 is OSD_OK."""
    lib = L.lib()
    p = C.c_void_p(4096)                                            # never dereferenced: the checks come first

    def call(src=p, ld_src=8, dst=p, ld_dst=8, rows=4, D=8, kind=p, knots=p, Q=16, levels=p, center=p, scale=p, inverse=0):
        return lib.osd_xf_apply(None, 0, src, ld_src, dst, ld_dst, rows, D, kind, knots, Q, levels, center, scale, inverse)

    assert call(rows=0) == L.OSD_OK
    for kw in ({"src": None}, {"dst": None}, {"kind": None}, {"knots": None}, {"levels": None}, {"center": None}, {"scale": None},
               {"Q": 1}, {"Q": 1025}, {"Q": 0}, {"D": 0}, {"D": -3}, {"rows": -1}, {"ld_src": 7}, {"ld_dst": 7}):
        assert call(**kw) == L.OSD_EINVAL, kw
        assert "bad argument" in L.last_error()
