"""CPU: the host side of ``pca.DevicePCA`` and ``BiologicalValidator.embedding_fidelity`` -- the subspace driver over the float64
NumPy kernels of tests/pca_helpers.py against sklearn, the planted samplers, checkpoints, argument errors, a gloo fit, and the new
entry points' place in the header and the ctypes table (the device kernels are tested in tests/test_gpu_pca.py)."""
import ctypes as C
import io
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import pca as PC
from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels
from pca_helpers import SAMPLERS, NumpyKernels, check_separations, cohort, planted_pair, project64, subspace64

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(600, 97, 5), (301, 130, 3), (2000, 515, 5)]


# ---- 1. the driver against sklearn ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,k", SHAPES)
def test_driver_matches_sklearn_full_svd(n, D, k):
    """Measured here (numpy 64-bit LAPACK, tol 1e-9): 14, 11 and 17 iterations; eigenvalues within 3.4e-15 relative, 1.6e-15 and
    3.2e-15 of sklearn's full SVD; 1 - |cos| of the components 4.5e-16, 3.4e-16, 5.6e-16.  The assertions are 4 x the largest."""
    x = cohort(n, D, k, 0)
    fit = PC.DevicePCA(k).fit(torch.from_numpy(x), kernels=NumpyKernels())
    from sklearn.decomposition import PCA
    sk = PCA(k, svd_solver="full").fit(x.astype(np.float64))
    dots = (fit.components_ * sk.components_).sum(1)
    eig = float(np.abs(fit.explained_variance_ / sk.explained_variance_ - 1.0).max())
    ang = float((1.0 - np.abs(dots)).max())
    print(f"n_iter {fit.n_iter_}  residual {fit.max_residual_:.3g}  eigenvalue gap {eig:.3g}  1 - |cos| {ang:.3g}")
    assert fit.converged_ and fit.n_iter_ <= 25 and fit.max_residual_ <= 1e-9
    assert eig <= 4 * 3.4e-15 and ang <= 4 * 5.6e-16
    assert (dots > 0).all()                                            # the signs are sklearn's
    assert np.abs(fit.explained_variance_ratio_ - sk.explained_variance_ratio_).max() <= 1e-14
    assert np.abs(fit.singular_values_ / sk.singular_values_ - 1.0).max() <= 1e-14
    assert np.abs(fit.mean_ - sk.mean_).max() <= 1e-14 and fit.n_samples_ == n and fit.constant_features_ == 0
    assert fit.components_.shape == (k, D) and fit.components_.dtype == np.float64
    # the plain driver of the helpers walks the same path from the same basis
    ref = subspace64(x, fit.initial_basis(D), k)
    assert ref["n_iter"] == fit.n_iter_ and ref["converged"]
    assert np.abs(ref["eigenvalues"] / fit.explained_variance_ - 1.0).max() <= 1e-13
    assert (1.0 - (ref["components"] * fit.components_).sum(1)).max() <= 1e-13


def test_standardize_matches_sklearn_on_scaled_columns_and_counts_constants():
    x = cohort(600, 97, 5, 0).copy()
    x[:, 3] *= 50.0
    x[:, 11] = 7.25
    fit = PC.DevicePCA(5, standardize=True).fit(torch.from_numpy(x), kernels=NumpyKernels())
    assert fit.constant_features_ == 1 and fit.scale_[11] == 0.0 and fit.converged_
    x64 = x.astype(np.float64)
    live = np.arange(97) != 11
    from sklearn.decomposition import PCA
    sk = PCA(5, svd_solver="full").fit((x64[:, live] - x64[:, live].mean(0)) / x64[:, live].std(0, ddof=1))
    assert np.abs(fit.explained_variance_ / sk.explained_variance_ - 1.0).max() <= 1e-12
    assert (1.0 - np.abs((fit.components_[:, live] * sk.components_).sum(1))).max() <= 1e-12
    assert np.abs(fit.components_[:, 11]).max() <= 1e-20               # W's row is exactly 0: what is left is the QR's rounding
    z = fit.transform(torch.from_numpy(x), kernels=NumpyKernels())
    assert z.dtype == torch.float32 and tuple(z.shape) == (600, 5)


def test_flat_spectrum_does_not_converge_and_does_not_raise():
    """The residual after 30 iterations measured here: 3.4e-4."""
    x = np.random.RandomState(3).randn(400, 60).astype(np.float32)
    fit = PC.DevicePCA(10, max_iter=30).fit(x, kernels=NumpyKernels())
    assert not fit.converged_ and fit.n_iter_ == 30 and 1e-9 < fit.max_residual_ < 1e-2
    assert np.all(np.diff(fit.explained_variance_) <= 0) and fit.components_.shape == (10, 60)
    assert np.abs(fit.components_ @ fit.components_.T - np.eye(10)).max() <= 1e-12


# ---- 2. the planted samplers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_planted_samplers_separate(kind):
    x, y = planted_pair(kind)
    rows = PC.embedding_rows(ShardComm(False), NumpyKernels(), torch.from_numpy(x), torch.from_numpy(y), 5)
    out = PC.embedding_summary(rows)
    check_separations(kind, out)
    assert out["pca_components"] == 5 and out["pca_converged"] is True and out["pca_constant_features"] == 0
    assert 0.40 < out["pca_explained_share_real"] < 0.48
    assert out["pca_variance_ratio_min"] <= out["pca_variance_ratio_mean"] <= out["pca_variance_ratio_max"]
    assert 1 <= out["pca_w1_scaled_max_component"] <= 5 and 0.0 <= out["pca_ks_mean"] <= out["pca_ks_max"] <= 1.0
    if kind == "noise":
        assert 1.5 < out["pca_residual_ratio"] < 1.9                  # 1.3^2 = 1.69
    if kind == "rotate":
        assert out["pca_captured_share_synth"] < 0.1
    # the captured share and the residuals restated from the fitted attributes
    real = rows["real"]
    z, n2 = project64(y, real.mean_, None, real.components_.T)
    assert out["pca_captured_share_synth"] == pytest.approx((z * z).sum() / n2.sum(), rel=1e-12)
    assert np.allclose(rows["synth_resid2"], np.maximum(n2 - (z * z).sum(1), 0.0), rtol=1e-9, atol=1e-9)
    assert out["pca_offmanifold_share"] == float((rows["synth_resid2"] > np.quantile(rows["real_resid2"], 0.99)).mean())


# ---- 3. checkpoints and argument errors -------------------------------------------------------------------------------------------
def test_state_round_trip_through_weights_only_load():
    x = cohort(301, 130, 3, 0)
    fit = PC.DevicePCA(3, standardize=True, seed=4).fit(x, kernels=NumpyKernels())
    buf = io.BytesIO()
    torch.save(fit.state(), buf)
    buf.seek(0)
    back = PC.DevicePCA.from_state(torch.load(buf, weights_only=True))
    for name in ("mean_", "scale_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_"):
        assert np.array_equal(getattr(back, name), getattr(fit, name)), name
    for name in ("n_samples_", "n_iter_", "converged_", "max_residual_", "constant_features_", "n_components", "oversample", "max_iter",
                 "tol", "standardize", "seed"):
        assert getattr(back, name) == getattr(fit, name), name
    k = NumpyKernels()
    a, ra = fit.transform(x, residual=True, kernels=k)
    b, rb = back.transform(x, residual=True, kernels=k)
    assert torch.equal(a, b) and torch.equal(ra, rb) and ra.dtype == torch.float64 and float(ra.min()) >= 0.0
    plain = PC.DevicePCA(3).fit(x, kernels=k)
    assert plain.state()["scale_"] is None and PC.DevicePCA.from_state(plain.state()).scale_ is None


def test_argument_errors():
    k = NumpyKernels()
    x = cohort(301, 130, 3, 0)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError):
            PC.DevicePCA(bad)
    for kw in ({"oversample": -1}, {"max_iter": 0}, {"tol": -1.0}):
        with pytest.raises(ValueError):
            PC.DevicePCA(3, **kw)
    with pytest.raises(ValueError, match="exceeds"):
        PC.DevicePCA(10).fit(x[:, :6], kernels=k)
    with pytest.raises(ValueError, match="at least 2"):
        PC.DevicePCA(2).fit(x[:1], kernels=k)
    hole = x.copy()
    hole[5, 7] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        PC.DevicePCA(2).fit(hole, kernels=k)
    with pytest.raises(ValueError):
        PC.DevicePCA(2).fit(x[0], kernels=k)
    with pytest.raises(RuntimeError):
        PC.DevicePCA(2).transform(x, kernels=k)
    with pytest.raises(RuntimeError):
        PC.DevicePCA(2).state()
    fit = PC.DevicePCA(2).fit(x, kernels=k)
    with pytest.raises(ValueError, match="features"):
        fit.transform(x[:, :100], kernels=k)
    rows = PC.embedding_rows(ShardComm(False), k, torch.from_numpy(x), torch.from_numpy(x), 2)
    with pytest.raises(ValueError):
        PC.embedding_summary(rows, quantile=1.5)
    # l = min(k + oversample, D, 32)
    assert PC.DevicePCA(10).initial_basis(5142).shape == (5142, 18) and PC.DevicePCA(30).initial_basis(100).shape == (100, 32)
    assert PC.DevicePCA(3).initial_basis(6).shape == (6, 6)
    v = PC.DevicePCA(4, seed=9).initial_basis(50)
    assert np.array_equal(v, np.linalg.qr(np.random.RandomState(9).randn(50, 12))[0])


def test_validator_refuses_a_cpu_device_and_bad_options():
    with pytest.raises(RuntimeError):
        BiologicalValidator({"evaluation": {}}, device="cpu")
    v = BiologicalValidator({"evaluation": {}}, device="cuda:0")
    with pytest.raises(ValueError, match="host.*device"):
        v.statistical_tests(np.zeros((4, 12), dtype=np.float32), np.zeros((4, 12), dtype=np.float32), pca="gpu")


# ---- 4. the entry points: declared, bound, and they check their arguments on the host ---------------------------------------------
def test_header_declares_and_lib_binds_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "osdiff.h").read_text(), flags=re.S)
    for name in ("osd_val_pca_project", "osd_val_pca_backproject"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert name in L.exported_symbols() and hasattr(L.lib(), name)
    assert int(re.search(r"#define\s+OSD_PCA_MAX_DIRS\s+(\d+)", text).group(1)) == L.OSD_PCA_MAX_DIRS == PC.MAX_DIRS == 32
    decl = re.search(r"int osd_val_pca_project\s*\((.*?)\);", text, flags=re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in decl.split(",")] == ["stream", "device", "X", "rows", "ld", "D", "center", "scale", "V", "l",
                                                                    "Z_dev", "norm2_dev"]
    assert len(L._SIGNATURES["osd_val_pca_project"][1]) == 12 and len(L._SIGNATURES["osd_val_pca_backproject"][1]) == 11
    for name in ("pca_project", "pca_backproject", "col_moments64"):
        assert callable(getattr(DeviceKernels, name))


def test_c_entry_points_refuse_bad_arguments_without_a_device():
    lib = L.lib()
    x = torch.zeros(64)
    d = torch.zeros(64, dtype=torch.float64)
    p = L.ptr
    proj = lambda X=p(x), rows=3, ld=8, D=8, c=p(d), V=p(d), l=2, Z=p(d), dev=0: lib.osd_val_pca_project(
        None, dev, X, rows, ld, D, c, None, V, l, Z, None)
    back = lambda X=p(x), rows=3, ld=8, D=8, c=p(d), Z=p(d), l=2, W=p(d), dev=0: lib.osd_val_pca_backproject(
        None, dev, X, rows, ld, D, c, None, Z, l, W)
    for call in (proj, back):
        assert call(l=0) == L.OSD_EINVAL and call(l=33) == L.OSD_EINVAL and call(l=9) == L.OSD_EINVAL          # l > D
        assert call(ld=32769, D=32769) == L.OSD_EINVAL and call(ld=7) == L.OSD_EINVAL
        assert call(rows=0) == L.OSD_EINVAL and call(rows=-5) == L.OSD_EINVAL and call(rows=2 ** 31) == L.OSD_EINVAL
        assert call(X=None) == L.OSD_EINVAL and call(c=None) == L.OSD_EINVAL and call(dev=-1) == L.OSD_EINVAL
        assert b"bad argument" in lib.osd_last_error()
    assert proj(V=None) == L.OSD_EINVAL and proj(Z=None) == L.OSD_EINVAL
    assert back(Z=None) == L.OSD_EINVAL and back(W=None) == L.OSD_EINVAL


# ---- 5. a fit over gloo equals the one-process fit --------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x = torch.from_numpy(cohort(301, 130, 3, 0))
        bounds = [0, 150, 301] if world == 2 else [0, 0, 120, 301]           # three ranks: the first shard is empty
        local = x[bounds[rank]:bounds[rank + 1]].contiguous()
        comm, k = ShardComm(True), NumpyKernels()
        assert comm.on and comm.world == world
        fit = PC.DevicePCA(3, standardize=(world == 3)).fit(local, comm=comm, kernels=k)
        one = PC.DevicePCA(3, standardize=(world == 3)).fit(x, kernels=k)
        ok = fit.n_samples_ == 301 and fit.converged_ and fit.n_iter_ == one.n_iter_
        ok &= float(np.abs(fit.explained_variance_ / one.explained_variance_ - 1.0).max()) <= 1e-12
        ok &= float((1.0 - (fit.components_ * one.components_).sum(1)).max()) <= 1e-12
        ok &= float(np.abs(fit.mean_ - one.mean_).max()) <= 1e-13
        ok &= abs(fit.explained_variance_ratio_.sum() / one.explained_variance_ratio_.sum() - 1.0) <= 1e-12
        q.put((rank, bool(ok), fit.explained_variance_.tobytes() + fit.components_.tobytes() + fit.mean_.tobytes()))
    except Exception as e:                           # report instead of leaving the parent to time out
        q.put((rank, repr(e), b""))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_fit_equals_single_process_gloo(world):
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
    assert sorted(r[:2] for r in res) == [(r, True) for r in range(world)]
    assert len({r[2] for r in res}) == 1                               # every rank ends with the same attributes, to the bit
