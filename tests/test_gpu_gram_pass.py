"""GPU: the host branches of the validator's Gram-pass entry points (csrc/validate.hip) that no other test pins directly: the RBF
sum on each of its three kernels and on its triangular schedule, osd_val_mmd against the three sums it is made of, the shared
row norms of a one-operand call, and the argument errors.

The RBF bound.  Per pair the fp32 expanded form |a|^2 + |b|^2 - 2 a.b is off by at most C_BOUND eps32 (|a|^2 + |b|^2) (C_BOUND
of tests/test_gpu_privacy.py, same row generator), which moves the exponent by gamma times that; expf and a lane's fp32 partial sum
of at most 64 terms <= 1 add at most 70 eps32 relative.  So

    |sum - sum64| <= sum_ij k64_ij (gamma C_BOUND eps32 (|a_i|^2 + |b_j|^2) + 70 eps32)

(a numpy fp32 restatement of the kernel sits at 0.05 % - 1 % of it on these inputs; the double slot sums add nothing visible)."""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.validation import DeviceKernels
from test_gpu_privacy import C_BOUND, EPS32, _rows

pytestmark = pytest.mark.gpu

RBF_SHAPES = [(130, 257, 70),      # ragged tiles, D % 4 != 0: the guarded kernel
              (130, 260, 68),      # D % 4 == 0, D % 32 != 0: the FAST kernel
              (256, 384, 64)]      # the LDS-DMA kernel


def _kernels():
    return DeviceKernels(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _pair(n, m, D):
    rs = np.random.default_rng(7000 + 100 * n + m + D)
    a, b = _rows(rs, n, D), _rows(rs, m, D) + np.float32(0.25)
    return a, b, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def _rbf64(a, b, gamma):
    """(sum, bound) of the module docstring: the float64 kernel sum over all pairs and what the device sum may be off by."""
    x, y = a.astype(np.float64), b.astype(np.float64)
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    norms = nx[:, None] + ny[None, :]
    k = np.exp(-gamma * np.maximum(norms - 2.0 * x @ y.T, 0.0))
    return float(k.sum()), float((k * (gamma * C_BOUND * EPS32 * norms + 70 * EPS32)).sum())


@pytest.mark.parametrize("n,m,D", RBF_SHAPES)
def test_rbf_sum_vs_float64(n, m, D):
    a, b, da, db = _pair(n, m, D)
    for gamma in (1.0 / D, 0.05):
        ref, bound = _rbf64(a, b, gamma)
        got = _kernels().rbf_sum(da, db, gamma)
        print(f"rbf_sum {n} x {m} x {D} gamma {gamma:.4g}: {got!r} vs {ref!r}, |diff| {abs(got - ref):.3e}, bound {bound:.3e}")
        assert abs(got - ref) <= bound


def test_rbf_sum_triangular_schedule():
    """One operand (same pointer, same rows): the upper-triangular tile schedule; a clone of it: the rectangle."""
    rs = np.random.default_rng(7300)
    a = _rows(rs, 300, 70)
    da = torch.from_numpy(a).cuda()
    for gamma in (1.0 / 70, 0.05):
        ref, bound = _rbf64(a, a, gamma)
        tri = _kernels().rbf_sum(da, da, gamma)
        rect = _kernels().rbf_sum(da, da.clone(), gamma)
        print(f"rbf_sum 300 x 70 gamma {gamma:.4g}: triangular {tri!r}, rectangle {rect!r}, float64 {ref!r}, bound {bound:.3e}")
        assert abs(tri - ref) <= bound and abs(rect - ref) <= bound and abs(tri - rect) <= bound


def _mmd(dx, dy, gamma):
    out = C_.c_double()
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().osd_val_mmd(stream, 0, L.ptr(dx), dx.shape[0], L.ptr(dy), dy.shape[0], dx.shape[1], float(gamma), C_.byref(out)))
    return float(out.value)


def test_mmd_is_its_three_sums():
    """osd_val_mmd and three osd_val_rbf_sum calls run the same kernels on the same row norms (X against itself on the triangular
    schedule in both), so their slot sums differ only in the order in which the workgroups' doubles arrive: a few hundred double
    additions per slot of terms that are <= 1 after the division by n^2, m^2 or n m -- 1e-13 at most; 1e-11 absolute is held."""
    n, m, D = RBF_SHAPES[0]
    _, _, dx, dy = _pair(n, m, D)
    k = _kernels()

    def recombined(gamma):
        sxx, syy, sxy = k.rbf_sum(dx, dx, gamma), k.rbf_sum(dy, dy, gamma), k.rbf_sum(dx, dy, gamma)
        return sxx / (float(n) * n) + syy / (float(m) * m) - 2.0 * sxy / (float(n) * m)

    for gamma, effective in ((0.05, 0.05), (0.0, 1.0 / D)):        # gamma = 0 picks 1 / D
        got, want = _mmd(dx, dy, gamma) ** 2, recombined(effective)
        print(f"mmd^2 gamma {gamma}: {got!r} vs recombined {want!r}, |diff| {abs(got - want):.3e}")
        assert want > 1e-4                                          # the two cohorts differ: the clamp at 0 is not what is compared
        assert abs(got - want) <= 1e-11
    assert abs(_mmd(dx, dy, 0.0) ** 2 - recombined(0.05)) > 1e-6   # and 1 / D is not 0.05: the two cases above are two cases


@pytest.mark.parametrize("n,D", [(257, 70), (256, 64)])
def test_shared_norms_bit_for_bit(n, D):
    """A one-operand call computes the row norms once and shares them; with a clone as the other operand they are computed twice.
    k_rowsumsq is deterministic and the keys and counts are order-independent integers: every output is the same bits."""
    rs = np.random.default_rng(7500 + n)
    x = torch.from_numpy(_rows(rs, n, D)).cuda()
    y = x.clone()
    own = torch.arange(n, dtype=torch.int32, device="cuda")
    k = _kernels()
    for name, call in (("nearest", lambda r: k.nearest(x, r, own)), ("knn", lambda r: k.knn(x, r, 5, own))):
        (d_s, i_s), (d_c, i_c) = call(x), call(y)
        assert torch.equal(i_s, i_c) and torch.equal(d_s.view(torch.int32), d_c.view(torch.int32)), name
        assert (i_s != own.view(-1, *([1] * (i_s.dim() - 1)))).all() and (i_s >= 0).all(), name
    r2 = k.knn(x, x, 5, own)[0][:, 4].contiguous()                  # every row's distance to its 5th neighbour
    (a_s, b_s), (a_c, b_c) = k.ball_counts(x, x, r2, r2), k.ball_counts(x, y, r2, r2)
    assert torch.equal(a_s, a_c) and torch.equal(b_s, b_c)
    assert (b_s >= 1).all() and (a_s >= 1).all()                    # a row lies inside its own ball: the counts are not all zero


def test_argument_errors_and_recovery():
    lib = L.lib()
    _, _, da, db = _pair(*RBF_SHAPES[0])
    n, m, D = RBF_SHAPES[0]
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = C_.c_double()

    def call(ap, an, bp, bn, gamma):
        return lib.osd_val_rbf_sum(stream, 0, ap, an, bp, bn, D, gamma, C_.byref(out))

    for bad in ((L.ptr(da), 0, L.ptr(db), m, 0.05), (None, n, L.ptr(db), m, 0.05), (L.ptr(da), n, None, m, 0.05),
                (L.ptr(da), n, L.ptr(db), m, 0.0), (L.ptr(da), n, L.ptr(db), m, -1.0)):
        assert call(*bad) == L.OSD_EINVAL
        assert b"bad argument" in lib.osd_last_error()
    assert call(L.ptr(da), n, L.ptr(db), m, 0.05) == L.OSD_OK       # the library stays usable
    ref, bound = _rbf64(*_pair(n, m, D)[:2], 0.05)
    assert abs(out.value - ref) <= bound
