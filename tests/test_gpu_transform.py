"""GPU: the feature-transform kernel (osd_xf_apply, csrc/transform.hip), ``FeatureTransform.forward`` / ``inverse`` above it and the
pipeline that carries a transform from ``prepare_data`` through the Trainer's checkpoint to the generator, against the float64
restatement of tests/transform_helpers.py evaluated on the same fp32 tables.

Kernel shapes (rows, D): (1, 1), (2, 5), (65, 33), (257, 130), (4099, 70), (7, 5142) and the ones that straddle the kernel's own
partition -- a strip is 32 columns, a workgroup takes 32 rows x 8 at a time, a row chunk is at least 512 rows: (256, 32) exactly one
strip and one pass; (257, 31) one row into the second pass, one column short of a strip ((257, 130) above is one row into it as well);
(513, 33) one row into the second chunk, one column into the second strip; (1025, 64) three chunks, two full strips.
Q in {2, 3, 100, 1000, 1024} (Q % 4 != 0 takes the scalar table load, the others the 16-byte one).  Each case runs dense, as an aligned and as an unaligned column slice of a wider matrix full of 1000s, out of place and in place, forward and
inverse.  The kinds are mixed so that they change inside strips and on strip boundaries (transform_helpers.SEGMENTS); the quantile
columns cycle through continuous, constant, subnormal-gap (2^-120 + i 2^-140), zero-inflated, half-integer (many plateaus) and
five-decade mixed-sign knots; the inputs through knots, midpoints, interior points, values below k[0] and above k[Q-1], +-inf and NaN.

  * bit equality wherever the rule returns a table entry, a mid-rank mean, a copy or NaN: clamps, knot hits, plateaus, identity;
  * |device - float64| <= 8 x 2^-23 x max(|a|, |b|), a and b the bracketing levels (forward) or knots (inverse), for an interpolated
    value: a + t (b - a) with t from two subtractions and a division is at most five fp32 roundings on values bounded by the bracket.
    A standard column: two roundings, 2 x 2^-23 x (|x| + |c|) / |s| forward and 2 x 2^-23 x (|z s| + |c|) inverse;
  * every inverse output of a quantile column lies inside [k[0], k[Q-1]]; inverse(forward(x)) == x bitwise for x at knots and on
    plateaus; one call equals two calls on halves; dense equals sliced; two calls return the same bits; bad arguments are OSD_EINVAL.

Measured on an MI355X (``pytest -s`` prints the figures): over all kernel cases the largest interpolation error was 0.48 of its bound
forward and 0.45 inverse, the figures an fp32 NumPy emulation of the rule gives; every exact entry matched in bits."""
import ctypes as C_

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator, load_trained_model
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.train import ResidentSplit, Trainer, prepare_data
from osteosarcoma_diffusionmodel_amd.transform import FeatureTransform
from transform_helpers import (QUANTILE, assert_matches, bits, make_case, reference, tiny_config, write_cohort)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 5), (65, 33), (257, 130), (4099, 70), (7, 5142), (256, 32), (257, 31), (513, 33), (1025, 64)]
QS = [2, 3, 100, 1000, 1024]
LAYOUTS = ["dense", "slice_aligned", "slice_unaligned"]


def _t(a):
    return torch.as_tensor(np.array(a)).cuda()                # a copy: the cached cases are read-only


def _layout(x, layout):
    """(view, whole): x on the device, dense or as a column slice of a wider matrix full of 1000s -- ld > D, neighbours must stay."""
    rows, D = x.shape
    if layout == "dense":
        t = _t(x)
        return t, t
    off = 1 if layout == "slice_unaligned" else 4
    width = (off + D + 8) // 4 * 4 + (1 if layout == "slice_unaligned" else 0)
    big = torch.full((rows, width), 1000.0, device="cuda")
    big[:, off:off + D] = _t(x)
    t = big[:, off:off + D]
    assert t.stride(0) == width > D and (t.data_ptr() % 16 == 0) == (layout == "slice_aligned")
    return t, big


def _neighbours_untouched(view, whole):
    if whole is view:
        return True
    off = (view.data_ptr() - whole.data_ptr()) // 4
    D = view.shape[1]
    return bool((whole[:, :off] == 1000.0).all()) and bool((whole[:, off + D:] == 1000.0).all())


class Tables:
    def __init__(self, case):
        self.kind, self.knots, self.levels = _t(case["kind"]), _t(case["knots"]), _t(case["levels"])
        self.center, self.scale = _t(case["center"]), _t(case["scale"])
        self.D, self.Q = case["D"], case["Q"]

    def rc(self, src, dst, inverse, /, **over):
        a = dict(rows=src.shape[0], D=self.D, Q=self.Q, ld_src=max(src.stride(0), self.D), ld_dst=max(dst.stride(0), self.D),
                 kind=self.kind, knots=self.knots, levels=self.levels, center=self.center, scale=self.scale, src=src, dst=dst)
        a.update(over)
        ptr = lambda v: L.ptr(v) if isinstance(v, torch.Tensor) or v is None else v
        stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.lib().osd_xf_apply(stream, 0, ptr(a["src"]), a["ld_src"], ptr(a["dst"]), a["ld_dst"], a["rows"], a["D"], ptr(a["kind"]),
                                  ptr(a["knots"]), a["Q"], ptr(a["levels"]), ptr(a["center"]), ptr(a["scale"]), 1 if inverse else 0)
        torch.cuda.synchronize()
        return rc

    def apply(self, src, dst, inverse):
        assert self.rc(src, dst, inverse) == L.OSD_OK, L.last_error()
        return dst


def _check_case(rows, D, Q, layout):
    case = make_case(rows, D, Q)
    (fref, fexact, ftol), (iref, iexact, itol) = reference(rows, D, Q)
    tb = Tables(case)
    qcols = np.flatnonzero(case["kind"] == QUANTILE)
    worst = {}
    for inverse, name, inp, ref, exact, tol in ((False, "forward", case["x"], fref, fexact, ftol), (True, "inverse", case["z"], iref, iexact, itol)):
        src, src_whole = _layout(inp, layout)
        dst, dst_whole = _layout(np.full((rows, D), -7.0, dtype=np.float32), layout)
        out = tb.apply(src, dst, inverse).cpu().numpy()
        what = f"{name} ({rows}, {D}) Q={Q} {layout}"
        worst[name] = assert_matches(out, ref, exact, tol, what)
        assert _neighbours_untouched(dst, dst_whole), f"{what}: a neighbour of dst was written"
        assert (bits(src.cpu().numpy()) == bits(inp)).all() and _neighbours_untouched(src, src_whole), f"{what}: src changed"
        inplace = tb.apply(src, src, inverse).cpu().numpy()
        assert (bits(inplace) == bits(out)).all(), f"{what}: in place differs from out of place"
        assert _neighbours_untouched(src, src_whole), f"{what}: in place wrote a neighbour"
        if inverse and qcols.size:
            o, k = out[:, qcols], case["knots"][qcols]
            ok = np.isnan(o) | ((o >= k[:, 0][None, :]) & (o <= k[:, -1][None, :]))
            assert ok.all(), f"{what}: an inverse value left its column's observed range"
    return worst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows, D", SHAPES)
def test_kernel_matches_the_rule(rows, D, layout):
    worst = _check_case(rows, D, 100, layout)
    print(f"\n({rows}, {D}) Q=100 {layout}: worst error / bound forward {worst['forward']:.4f}, inverse {worst['inverse']:.4f}")


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("rows, D", [(65, 33), (257, 130)])
def test_kernel_matches_the_rule_over_Q(rows, D, Q):
    for layout in (LAYOUTS if (rows, D) == (65, 33) else ["dense"]):
        worst = _check_case(rows, D, Q, layout)
        print(f"\n({rows}, {D}) Q={Q} {layout}: worst error / bound forward {worst['forward']:.4f}, inverse {worst['inverse']:.4f}")


def test_chunk_straddle_at_the_largest_table():
    """Q = 1024: 132 KiB of tables, one workgroup per CU, on a shape one row into the second chunk and one column into the second strip."""
    worst = _check_case(513, 33, 1024, "slice_unaligned")
    print(f"\n(513, 33) Q=1024: worst error / bound forward {worst['forward']:.4f}, inverse {worst['inverse']:.4f}")


def test_wide_matrix_at_a_thousand_levels():
    worst = _check_case(7, 5142, 1000, "slice_unaligned")
    print(f"\n(7, 5142) Q=1000: worst error / bound forward {worst['forward']:.4f}, inverse {worst['inverse']:.4f}")


@pytest.mark.parametrize("Q", [3, 100, 1024])
def test_round_trip(Q):
    """inverse(forward(x)) == x bitwise for x at knots and on plateaus.  For interior points the round trip is two interpolations: the
    largest |inverse(forward(x)) - x| relative to the local knot gap is printed.  Measured on an MI355X: 1.835e-07 at Q = 3, 2.167e-06
    at Q = 100, 2.556e-05 at Q = 1024 (the narrow level gaps in the middle of a long table amplify the rounding of z)."""
    D = 130
    case = make_case(Q, D, Q)
    tb = Tables(case)
    qcols = np.flatnonzero(case["kind"] == QUANTILE)
    at_knots = np.array(case["x"])
    at_knots[:, qcols] = case["knots"][qcols].T                 # row i holds knot i of every quantile column
    at_knots[~np.isfinite(at_knots)] = 0.5
    x = _t(at_knots)
    back = tb.apply(tb.apply(x, torch.empty_like(x), False), torch.empty_like(x), True).cpu().numpy()
    assert (bits(back[:, qcols]) == bits(at_knots[:, qcols])).all()
    ident = np.flatnonzero(case["kind"] == 0)
    assert (bits(back[:, ident]) == bits(at_knots[:, ident])).all()
    # interior points: u of the way from knot j to knot j + 1, in units of that gap
    rs = np.random.default_rng(Q)
    k = case["knots"][qcols].astype(np.float64)                 # [columns, Q]
    j = rs.integers(0, Q - 1, (Q, qcols.size))
    u = rs.uniform(0.05, 0.95, (Q, qcols.size))
    lo, hi = np.take_along_axis(k.T, j, axis=0), np.take_along_axis(k.T, j + 1, axis=0)
    inner = np.array(at_knots)
    inner[:, qcols] = (lo + u * (hi - lo)).astype(np.float32)
    x = _t(inner)
    back = tb.apply(tb.apply(x, torch.empty_like(x), False), torch.empty_like(x), True).cpu().numpy()
    gap = hi - lo
    live = gap > 0
    err = np.abs(back[:, qcols].astype(np.float64) - inner[:, qcols].astype(np.float64))
    assert (err[~live] == 0).all()                              # a point on a plateau is the plateau
    rel = float((err[live] / gap[live]).max()) if live.any() else 0.0
    print(f"\nround trip Q={Q}: largest |inverse(forward(x)) - x| / local knot gap = {rel:.3e}")
    assert np.isfinite(back[:, qcols]).all()


def test_geometry_independence_layouts_and_repeats():
    """One call on n rows equals two calls on halves (other chunk boundaries, other passes), dense equals sliced, and a second call
    returns the same bits."""
    rows, D, Q = 1025, 64, 100
    case = make_case(rows, D, Q)
    tb = Tables(case)
    for inverse, inp in ((False, case["x"]), (True, case["z"])):
        whole = tb.apply(_t(inp), torch.empty(rows, D, device="cuda"), inverse).cpu().numpy()
        again = tb.apply(_t(inp), torch.empty(rows, D, device="cuda"), inverse).cpu().numpy()
        assert (bits(whole) == bits(again)).all()
        h = 512
        a = tb.apply(_t(inp[:h]), torch.empty(h, D, device="cuda"), inverse).cpu().numpy()
        b = tb.apply(_t(inp[h:]), torch.empty(rows - h, D, device="cuda"), inverse).cpu().numpy()
        assert (bits(np.concatenate([a, b])) == bits(whole)).all()
        for layout in ("slice_aligned", "slice_unaligned"):
            src, _ = _layout(inp, layout)
            dst, _ = _layout(np.zeros((rows, D), dtype=np.float32), layout)
            assert (bits(tb.apply(src, dst, inverse).cpu().numpy()) == bits(whole)).all(), layout


def test_bad_arguments_are_einval_without_a_launch():
    case = make_case(65, 33, 100)
    tb = Tables(case)
    src = _t(case["x"])
    dst = torch.full((65, 33), -7.0, device="cuda")
    for over in ({"src": None}, {"dst": None}, {"kind": None}, {"knots": None}, {"levels": None}, {"center": None}, {"scale": None},
                 {"Q": 1}, {"Q": 1025}, {"D": 0}, {"rows": -1}, {"ld_src": 32}, {"ld_dst": 32}):
        assert tb.rc(src, dst, False, **over) == L.OSD_EINVAL, over
    bad = np.array(case["kind"])
    bad[17] = 3
    assert tb.rc(src, dst, False, kind=_t(bad)) == L.OSD_EINVAL and "kind[17] = 3" in L.last_error()
    bad[17] = -1
    assert tb.rc(src, dst, True, kind=_t(bad)) == L.OSD_EINVAL
    assert bool((dst == -7.0).all())                            # nothing was launched
    assert tb.rc(src, dst, False, rows=0) == L.OSD_OK and bool((dst == -7.0).all())


def test_feature_transform_methods():
    """``FeatureTransform.forward`` / ``inverse``: the fitted tables on the device, a row stride honoured, in place, and ``forward_host``
    (what ``map_bounds`` evaluates) equal to the kernel bit for bit."""
    rs = np.random.default_rng(3)
    blocks = {"mutations": 4, "expression": 40, "pathways": 6}
    n = 300
    x = np.concatenate([rs.integers(0, 2, (n, 4)), np.where(rs.random((n, 40)) < 0.3, 0.0, np.exp(rs.normal(1, 1, (n, 40)))),
                        rs.normal(1, 2, (n, 6))], axis=1).astype(np.float32)
    ft = FeatureTransform.fit(x, blocks, {"expression": "quantile_normal", "pathways": "standard"}, n_quantiles=128)
    xd = _t(x)
    z = ft.forward(xd)
    assert z.shape == xd.shape and z.dtype == torch.float32 and torch.equal(xd.cpu(), torch.from_numpy(x))
    host = np.stack([ft.forward_host(row) for row in x[:40]])
    assert (bits(z[:40].cpu().numpy()) == bits(host)).all()
    assert torch.equal(z[:, :4], xd[:, :4])
    # the data's own values are knots or lie on plateaus when Q = n; at Q = 128 < n they come back within the interpolation error, and
    # exactly inside the observed range
    back = ft.inverse(z)
    k = ft.knots.numpy()[4:44]
    b = back[:, 4:44].cpu().numpy()
    assert ((b >= k[:, 0][None, :]) & (b <= k[:, -1][None, :])).all() and (b >= 0).all()
    wide = torch.full((n, 64), 1000.0, device="cuda")
    view = wide[:, 3:53]
    view.copy_(xd)
    assert ft.forward(view, out=view) is view and torch.equal(view, z)
    assert bool((wide[:, :3] == 1000.0).all()) and bool((wide[:, 53:] == 1000.0).all())
    nan = xd.clone()
    nan[::3, 5:] = float("nan")
    zn = ft.forward(nan)
    assert torch.equal(torch.isnan(zn), torch.isnan(nan)) and torch.equal(zn[~torch.isnan(nan)], z[~torch.isnan(nan)])
    assert ft.forward(xd[:0]).shape == (0, 50)
    with pytest.raises(ValueError, match="out must be"):
        ft.forward(xd, out=torch.empty(n, 50, device="cuda", dtype=torch.float64))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
TRANSFORM = {"expression": "quantile_normal", "pathways": "standard", "n_quantiles": 1000}
SCENARIO = {"survival_time": 600, "event_occurred": 1, "age": 14.0, "metastasis_at_diagnosis": 0}


def _train(root, transform):
    processed = root / "processed"
    frames = write_cohort(processed)
    conf = tiny_config(processed, root / "ckpt", transform)
    train_loader, val_loader, conf = prepare_data(conf)
    m = conf["model"]
    torch.manual_seed(0)
    model = BiologyAwareDiffusionModel(m["n_genes_mutation"], m["n_genes_expression"], m["n_pathways"], m["n_conditions"], conf)
    tr = Trainer(model, train_loader, val_loader, conf, device="cuda")
    for i, batch in enumerate(train_loader):
        if i == 2:
            break
        tr.train_step(batch["data"].cuda(), batch["conditions"].cuda(), seed=100 + i)
    tr.save_checkpoint(0, 1.0)
    return {"frames": frames, "processed": processed, "conf": conf, "train_loader": train_loader, "trainer": tr, "model": model,
            "ckpt": root / "ckpt" / "checkpoint_epoch_0.pt"}


@pytest.fixture(scope="module")
def with_transform(tmp_path_factory):
    return _train(tmp_path_factory.mktemp("xf"), TRANSFORM)


@pytest.fixture(scope="module")
def without_transform(tmp_path_factory):
    return _train(tmp_path_factory.mktemp("plain"), None)


def _reference_matrix(processed):
    """The reference's [mutations | expression | z-scored pathways] matrix, read back from the CSVs as ``prepare_data`` reads them."""
    import pandas as pd
    mut, expr, pw = (pd.read_csv(processed / f, index_col=0) for f in ("mutation_matrix_aligned.csv", "expression_matrix_aligned.csv",
                                                                       "pathway_scores.csv"))
    pw = (pw - pw.mean()) / (pw.std() + 1e-8)
    return torch.cat([torch.FloatTensor(f.values.astype(np.float32)) for f in (mut, expr, pw)], dim=1)


def test_prepare_data_fits_on_the_training_rows_and_maps_on_the_device(with_transform, without_transform):
    run = with_transform
    base, rows = ResidentSplit._base_of(run["train_loader"].dataset)
    ft = base.feature_transform
    raw = _reference_matrix(run["processed"])
    assert torch.equal(base.raw_data, raw)
    assert rows.numel() == 160 and ft.levels.shape[0] == 160 and ft.blocks == {"mutations": 6, "expression": 30, "pathways": 4}
    refit = FeatureTransform.fit(raw[rows], ft.blocks, {"expression": "quantile_normal", "pathways": "standard"}, n_quantiles=1000)
    for name in ("kind", "knots", "levels", "center", "scale"):
        assert torch.equal(getattr(ft, name), getattr(refit, name)), name
    assert torch.equal(base.data, ft.forward(raw.cuda()).cpu())
    assert torch.equal(base.data[:, :6], raw[:, :6])
    z = base.data[rows][:, 6:36].numpy().astype(np.float64)
    assert np.abs(z.mean(0)).max() < 0.35 and np.abs(z.std(0) - 1).max() < 0.35          # Gaussianised, zeros at their mid-rank
    assert run["model"].feature_transform is ft
    # absent: the reference's matrix and no new attribute
    plain, _ = ResidentSplit._base_of(without_transform["train_loader"].dataset)
    assert torch.equal(plain.data, raw) and not hasattr(plain, "feature_transform") and not hasattr(plain, "raw_data")
    assert without_transform["model"].feature_transform is None


def test_checkpoint_carries_the_transform_and_generate_speaks_data_units(with_transform):
    run = with_transform
    conf = run["conf"]
    ckpt = torch.load(run["ckpt"], map_location="cpu", weights_only=True)
    assert "feature_transform" in ckpt and set(ckpt["feature_transform"]) >= {"kind", "knots", "levels", "center", "scale", "blocks", "spec"}
    model = load_trained_model(run["ckpt"], conf, "cuda")
    ft = model.feature_transform
    assert torch.equal(ft.knots, run["model"].feature_transform.knots) and ft.spec == run["model"].feature_transform.spec
    with pytest.raises(ValueError, match="data.*transform"):
        load_trained_model(run["ckpt"], {**conf, "data": {**conf["data"], "transform": {"expression": "standard"}}}, "cuda")
    gen = SyntheticPatientGenerator(model, conf, device="cuda")
    out = gen.generate(64, SCENARIO, seed=11, sampling_steps=5)
    cond = gen.create_conditions(64, SCENARIO)
    z, mask = model.sample(cond, 64, seed=11, num_inference_steps=5, return_mutation_mask=True)
    want = ft.inverse(z).cpu().numpy()
    got = np.concatenate([out["mutations"], out["expression"], out["pathways"]], axis=1)
    assert (bits(out["expression"]) == bits(want[:, 6:36])).all() and (bits(out["pathways"]) == bits(want[:, 36:])).all()
    assert (out["mutations"] == mask.cpu().numpy()).all() and got.shape == (64, 40)
    k = ft.knots.numpy()[6:36]
    assert ((out["expression"] >= k[:, 0][None, :]) & (out["expression"] <= k[:, -1][None, :])).all() and (out["expression"] >= 0).all()
    both = gen.generate_scenarios([{"name": "a", "conditions": SCENARIO}, {"name": "b", "conditions": {**SCENARIO, "event_occurred": 0}}],
                                  16, seed=3, sampling_steps=5)
    for part in both.values():
        assert ((part["expression"] >= k[:, 0][None, :]) & (part["expression"] <= k[:, -1][None, :])).all()


def test_known_impute_and_bounds_in_data_units(with_transform):
    run = with_transform
    conf = run["conf"]
    model = load_trained_model(run["ckpt"], conf, "cuda")
    ft = model.feature_transform
    gen = SyntheticPatientGenerator(model, conf, device="cuda")
    base, rows = ResidentSplit._base_of(run["train_loader"].dataset)
    n = 32
    feats = base.raw_data[rows[:n]].clone().numpy()
    feats[:, 10] = np.float32(0.75)                                 # between two knots and off every table: only the restore keeps it
    feats[:, 20] *= np.float32(1.0001)
    holes = np.random.default_rng(0).random(feats.shape) < 0.4
    holes[:, 36:] = True                                            # no pathway observed
    observed = np.where(holes, np.nan, feats).astype(np.float32)
    cond = base.conditions[rows[:n]]
    out = gen.impute(observed, cond, seed=5, sampling_steps=5)
    got = np.concatenate([out["mutations"], out["expression"], out["pathways"]], axis=1)
    assert np.isfinite(got).all()
    assert (bits(got[:, 6:][~holes[:, 6:]]) == bits(observed[:, 6:][~holes[:, 6:]])).all()          # observed values come back exactly
    assert (out["mutations"][~holes[:, :6]] == (observed[:, :6][~holes[:, :6]] > 0.5)).all()
    # the chain ran around the forward-mapped observations
    kn = ft.forward(torch.from_numpy(observed).cuda())
    z = model.sample(cond.cuda(), n, seed=5, num_inference_steps=5, known=kn)
    want = ft.inverse(z).cpu().numpy()
    assert (bits(got[:, 6:][holes[:, 6:]]) == bits(want[:, 6:][holes[:, 6:]])).all()
    # known= through generate: one observed row broadcast to all samples
    one = gen.generate(8, SCENARIO, seed=2, sampling_steps=5, known={"expression": observed[:1, 6:36]})
    seen = ~np.isnan(observed[0, 6:36])
    assert (bits(one["expression"][:, seen]) == bits(np.broadcast_to(observed[0, 6:36][seen], (8, int(seen.sum()))))).all()
    assert np.isfinite(one["expression"]).all()
    # x0_bounds in data units = model.sample with the hand-mapped bounds
    spec = {"expression": (0.5, 9.0), "pathways": (-1.0, None)}
    data_units = gen.generate(16, SCENARIO, seed=7, sampling_steps=5, x0_bounds=spec)
    from osteosarcoma_diffusionmodel_amd.generate import assemble_bounds
    lo, hi = ft.map_bounds(*assemble_bounds(spec, 6, 30, 4))
    assert np.isposinf(hi[36:]).all() and np.isneginf(lo[:6]).all() and np.isfinite(lo[6:]).all()
    data_lo = assemble_bounds(spec, 6, 30, 4)[0]
    dev_lo = ft.forward(torch.from_numpy(np.where(np.isfinite(data_lo), data_lo, np.float32(0)))[None, :].cuda())[0].cpu().numpy()
    assert (bits(dev_lo[6:]) == bits(lo[6:])).all()                 # the host map of the bounds is the kernel's, bit for bit
    z = model.sample(gen.create_conditions(16, SCENARIO), 16, seed=7, num_inference_steps=5, x0_bounds=(lo, hi))
    want = ft.inverse(z).cpu().numpy()
    assert (bits(data_units["expression"]) == bits(want[:, 6:36])).all() and (bits(data_units["pathways"]) == bits(want[:, 36:])).all()
    # inside the bounds up to the round trip of the bound itself (two interpolations: a few fp32 roundings of values below 16)
    slack = 16 * 2.0 ** -20
    assert (data_units["expression"] >= 0.5 - slack).all() and (data_units["expression"] <= 9.0 + slack).all()
    assert (data_units["pathways"] >= -1.0 - slack).all()


def test_without_a_transform_nothing_changes(without_transform):
    run = without_transform
    conf = run["conf"]
    ckpt = torch.load(run["ckpt"], map_location="cpu", weights_only=True)
    assert "feature_transform" not in ckpt
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "config"}
    model = load_trained_model(run["ckpt"], conf, "cuda")
    assert model.feature_transform is None
    gen = SyntheticPatientGenerator(model, conf, device="cuda")
    out = gen.generate(64, SCENARIO, seed=11, sampling_steps=5)
    z = model.sample(gen.create_conditions(64, SCENARIO), 64, seed=11, num_inference_steps=5).cpu().numpy()
    assert (bits(out["expression"]) == bits(z[:, 6:36])).all() and (bits(out["pathways"]) == bits(z[:, 36:])).all()


def test_membership_audit_takes_data_units(with_transform):
    from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator
    run = with_transform
    model = load_trained_model(run["ckpt"], run["conf"], "cuda")
    ft = model.feature_transform
    base, rows = ResidentSplit._base_of(run["train_loader"].dataset)
    train = (base.raw_data[rows[:48]], base.conditions[rows[:48]])
    hold = (base.raw_data[rows[48:80]], base.conditions[rows[48:80]])
    v = BiologicalValidator({"evaluation": {}}, device="cuda")
    res = v.membership_audit(model, train, hold, num_timesteps=4, seed=1)
    want = model.variational_bound(ft.forward(train[0].cuda()), train[1].cuda(), num_timesteps=4, seed=1, row_offset=0)["bpd"]
    assert res["mean_bpd_train"] == float(want.cpu().numpy().mean())


def test_trainer_holds_model_and_dataset_to_one_transform(with_transform, without_transform):
    """A model that already carries a map (a loaded checkpoint) trains only on data that went through the same one, and a checkpoint
    resumes only behind the map it was written behind."""
    run, plain = with_transform, without_transform
    base, rows = ResidentSplit._base_of(run["train_loader"].dataset)
    loaded = load_trained_model(run["ckpt"], run["conf"], "cuda")
    assert loaded.feature_transform is not base.feature_transform and loaded.feature_transform.same_as(base.feature_transform)
    tr = Trainer(loaded, run["train_loader"], run["train_loader"], run["conf"], device="cuda")
    assert loaded.feature_transform is base.feature_transform
    assert tr.load_checkpoint(run["ckpt"]) == 0 and loaded.feature_transform.same_as(base.feature_transform)
    with pytest.raises(ValueError, match="trained without data.transform"):
        tr.load_checkpoint(plain["ckpt"])
    with pytest.raises(ValueError, match="prepared without data.transform"):
        plain["trainer"].load_checkpoint(run["ckpt"])
    assert plain["model"].feature_transform is None
    with pytest.raises(ValueError, match="prepared without data.transform"):
        Trainer(load_trained_model(run["ckpt"], run["conf"], "cuda"), plain["train_loader"], plain["train_loader"], plain["conf"], device="cuda")
    other = BiologyAwareDiffusionModel(6, 30, 4, 4, run["conf"])
    other.feature_transform = FeatureTransform.fit(base.raw_data[rows[:100]], base.feature_transform.blocks,
                                                   {"expression": "quantile_normal", "pathways": "standard"}, n_quantiles=1000)
    with pytest.raises(ValueError, match="differs from the dataset's data.transform"):
        Trainer(other, run["train_loader"], run["train_loader"], run["conf"], device="cuda")


def test_refusals_on_the_device(with_transform, tmp_path):
    run = with_transform
    model = run["model"]
    with pytest.raises(ValueError, match="data.transform"):
        model.set_constraints(pathways=[[6, 7, 8]])
    from osteosarcoma_diffusionmodel_amd.cvae import BiologyConstrainedVAE
    conf = {**run["conf"], "model": {**run["conf"]["model"], "architecture": "cvae",
                                     "constraints": {"pathway_coherence_weight": 1.0, "mutation_expression_weight": 0.5,
                                                     "survival_prediction_weight": 0.3}}}
    vae = BiologyConstrainedVAE(6, 30, 4, 4, conf)
    with pytest.raises(ValueError, match="data.transform.*cVAE"):
        Trainer(vae, run["train_loader"], run["train_loader"], run["conf"], device="cuda")
    plain = BiologyAwareDiffusionModel(6, 30, 4, 4, run["conf"])
    plain.set_constraints(pathways=[[6, 7, 8]])
    with pytest.raises(ValueError, match="data.transform.*constraint losses"):
        Trainer(plain, run["train_loader"], run["train_loader"], run["conf"], device="cuda")
