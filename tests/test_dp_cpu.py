"""CPU: differentially private training without a device -- the float64 oracle's vectorised form against its brute-force definition,
the accountant (privacy.py) against a closed form, a quadrature and its own monotonicity, and every ValueError of ``training.dp``."""
import math

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd import privacy as PV
from osteosarcoma_diffusionmodel_amd.train import Trainer
from helpers import config
from loss_helpers import P_DROP, inputs
from dp_helpers import DpOracle, choose_C, moment_quadrature

H3 = [256, 512, 256]
DIMS = (6, 83, 4, 4)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("kind, prediction, drop", [("l2", "epsilon", True), ("huber", "v_prediction", False)])
def test_vectorised_oracle_equals_brute_force(kind, prediction, drop):
    """n = 6: the row-norm identity's s_r and the weighted-loss gradient equal one autograd.grad per row, to 1e-10 relative."""
    n = 6
    sd, x, cond, t, noise, injected = inputs(DIMS, H3, n)
    weights = None if kind == "l2" else torch.rand(1000, generator=torch.Generator().manual_seed(3)) + 0.5
    orc = DpOracle(sd, x, cond, t, noise, H3, injected if drop else None, P_DROP, kind=kind, delta=0.7, weights=weights, prediction=prediction)
    fast = orc.norms()
    C = float(np.median(fast.numpy()))
    slow, g_slow = orc.brute(C)
    print(f"norms {fast.numpy()}  C {C}")
    assert (fast > C).any() and (fast < C).any()
    assert _rel(fast, slow) <= 1e-10
    g_fast = orc.clipped(C)
    for k in g_slow:
        assert _rel(g_fast[k], g_slow[k]) <= 1e-10, k
    # C beyond every norm: the plain gradient of the mean loss
    _, plain = orc.orc.grads_of(lambda pd: orc._rows(pd).mean())
    for k, g in orc.clipped(1e30).items():
        assert _rel(g, plain[k]) <= 1e-12, k


def test_choose_c_moves_off_a_row():
    assert choose_C([1.0, 2.0, 3.0, 4.0]) == 2.5
    c = choose_C([1.0, 2.0, 3.0, 4.0, 5.0])          # the median is a row's norm: C moves into a gap next to it
    assert c in (2.5, 3.5)
    with pytest.raises(AssertionError):
        choose_C([1.0] * 7 + [5.0])                   # one row of eight clipped once C sits in the only gap: fewer than a quarter


# ---- the accountant ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma, T", [(1.0, 1), (2.0, 100), (4.0, 1000)])
def test_accountant_closed_form_at_q1(sigma, T):
    """q = 1 is the plain Gaussian mechanism: eps_R(alpha) = alpha / (2 sigma^2) exactly, so the continuous-order optimum of the
    conversion is T / (2 sigma^2) + sqrt(2 T ln(1/delta)) / sigma; the order grid lies above it, by at most 2 %."""
    delta = 1e-5
    for a in (1.5, 2.0, 7.25, 64.0):
        assert PV.log_moment(1.0, sigma, a) / (a - 1.0) == pytest.approx(a / (2 * sigma ** 2), rel=1e-14)
    bound = T / (2 * sigma ** 2) + math.sqrt(2 * T * math.log(1 / delta)) / sigma
    eps = PV.epsilon(1.0, sigma, T, delta)
    print(f"sigma {sigma} T {T}: grid {eps:.6f} continuous {bound:.6f} (+{eps / bound - 1:.2e})")
    assert bound * (1 - 1e-12) <= eps <= 1.02 * bound


@pytest.mark.parametrize("alpha", [2, 3, 8, 32])
@pytest.mark.parametrize("q", [0.01, 0.1, 0.5])
def test_accountant_moment_vs_quadrature(alpha, q):
    for sigma in (1.0, 2.0):
        got, ref = PV.log_moment(q, sigma, alpha), moment_quadrature(q, sigma, alpha)
        assert abs(got - ref) <= 1e-8 * abs(ref), (alpha, q, sigma, got, ref)


@pytest.mark.parametrize("alpha", [1.5, 2.5, 7.3])
def test_accountant_fractional_orders_vs_quadrature(alpha):
    """The fractional orders' series (not exercised at q = 1) against the same quadrature."""
    for q in (0.01, 0.1, 0.5):
        got, ref = PV.log_moment(q, 1.3, alpha), moment_quadrature(q, 1.3, alpha)
        assert abs(got - ref) <= 1e-8 * abs(ref), (alpha, q, got, ref)


def test_accountant_behaviour():
    base = PV.epsilon(0.02, 1.1, 500, 1e-5)
    assert 0 < base < float("inf")
    assert PV.epsilon(0.02, 1.1, 1000, 1e-5) > base          # more steps
    assert PV.epsilon(0.04, 1.1, 500, 1e-5) > base           # a larger sample rate
    assert PV.epsilon(0.02, 1.5, 500, 1e-5) < base           # more noise
    assert PV.epsilon(0.02, 1.1, 0, 1e-5) == 0.0 and PV.epsilon(0.02, 0.0, 10, 1e-5) == float("inf")
    for target, q, T in ((1.0, 0.01, 2000), (8.0, 0.2, 50)):
        sigma = PV.noise_multiplier_for(target, q, T, 1e-5)
        back = PV.epsilon(q, sigma, T, 1e-5)
        print(f"target {target}: sigma {sigma:.4f} -> epsilon {back:.4f}")
        assert back <= target and abs(back - target) <= 0.01 * target


# ---- training.dp: every ValueError before a device is touched ----------------------------------------------------------------------
def _conf(tmp_path, dp, mixup=0.0):
    conf = config(H3, p=0.0)
    conf["training"] = {"learning_rate": 1e-3, "weight_decay": 1e-5, "patience": 5, "min_delta": 1e-4, "augmentation": {"mixup_alpha": mixup},
                        "save_dir": str(tmp_path), "num_epochs": 2, "save_frequency": 10, "val_split": 0.2, "random_seed": 1, "batch_size": 8,
                        "dp": dp}
    return conf


def _model(conf):
    return BiologyAwareDiffusionModel(config=conf, mutation_dim=6, expression_dim=83, pathway_dim=4, condition_dim=4)


GOOD = {"max_grad_norm": 1.0, "noise_multiplier": 1.1, "delta": 1e-5}
BAD = {
    "both": ({**GOOD, "target_epsilon": 3.0}, "exactly one"),
    "neither": ({"max_grad_norm": 1.0}, "exactly one"),
    "zero C": ({**GOOD, "max_grad_norm": 0.0}, "max_grad_norm"),
    "negative C": ({**GOOD, "max_grad_norm": -1.0}, "max_grad_norm"),
    "no C": ({"noise_multiplier": 1.0}, "max_grad_norm"),
    "negative sigma": ({**GOOD, "noise_multiplier": -0.1}, "noise_multiplier"),
    "delta": ({**GOOD, "delta": 1.5}, "delta"),
    "unknown key": ({**GOOD, "clip": 1.0}, "unknown"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_config_value_errors(case, tmp_path, monkeypatch):
    monkeypatch.setattr(torch.nn.Module, "to", lambda *a, **k: pytest.fail("the model was moved to a device before validation"))
    dp, match = BAD[case]
    conf = _conf(tmp_path, dp)
    with pytest.raises(ValueError, match=match):
        Trainer(_model(conf), [], [], conf, device="cuda")


def test_config_refuses_mixup_constraints_cvae_and_data_parallel(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.nn.Module, "to", lambda *a, **k: pytest.fail("the model was moved to a device before validation"))
    conf = _conf(tmp_path, dict(GOOD), mixup=0.2)
    with pytest.raises(ValueError, match="mixup_alpha.*0.2"):          # says how to fix it, and that the reference's default is on
        Trainer(_model(conf), [], [], conf, device="cuda")
    conf = _conf(tmp_path, dict(GOOD))
    m = _model(conf)
    m.set_constraints(pathways=[[7, 8, 9]], pathway_weight=0.5)
    with pytest.raises(ValueError, match="constraint"):
        Trainer(m, [], [], conf, device="cuda")

    class FakeVae(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.vae = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="cVAE"):
        Trainer(FakeVae(), [], [], conf, device="cuda")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda: 2)
    with pytest.raises(ValueError, match="data parallel"):
        Trainer(_model(conf), [], [], conf, device="cuda")


def test_target_epsilon_needs_planned_steps_before_the_device(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.nn.Module, "to", lambda *a, **k: pytest.fail("the model was moved to a device before validation"))
    conf = _conf(tmp_path, {"max_grad_norm": 1.0, "target_epsilon": 3.0})
    with pytest.raises(ValueError, match="planned step"):
        Trainer(_model(conf), [], [], conf, device="cuda")          # an empty loader: num_epochs x 0 batches


def test_check_dp_config_accepts():
    tc = {"augmentation": {"mixup_alpha": 0.0}}
    assert PV.check_dp_config(None, tc) is None
    got = PV.check_dp_config({"max_grad_norm": 2, "noise_multiplier": 0}, tc)          # clipping only: epsilon = inf
    assert got == {"max_grad_norm": 2.0, "noise_multiplier": 0.0, "target_epsilon": None, "delta": 1e-5, "seed": None}
    got = PV.check_dp_config({"max_grad_norm": 0.5, "target_epsilon": 3, "delta": 1e-6, "seed": 7}, tc)
    assert got["noise_multiplier"] is None and got["target_epsilon"] == 3.0 and got["seed"] == 7
