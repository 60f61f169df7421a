"""CPU: the host side of fine-tuning -- the group-table builder, transfer.load_pretrained on nn modules, the NumPy restatement of the
grouped step against torch.optim.AdamW, the argument checks of the two grouped entry points, and the Trainer's refusals.  No device."""
import copy
import ctypes as C
import json
import logging

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, _lib as L, load_pretrained
from osteosarcoma_diffusionmodel_amd.cvae import BiologyConstrainedVAE
from osteosarcoma_diffusionmodel_amd.train import Trainer, build_param_groups, merge_param_groups
from helpers import SM, SM_H, config
import transfer_helpers as TH

NAMES = ["condition_embed.mlp.0.weight", "condition_embed.mlp.0.bias", "unet.time_proj.weight", "unet.input_proj.weight",
         "unet.encoder.0.weight", "unet.encoder.0.bias", "unet.encoder.1.weight", "unet.encoder2.weight", "unet.decoder.0.weight",
         "unet.output_proj.weight"]


# ---- the group-table builder ----------------------------------------------------------------------------------------------------------
def test_builder_longest_prefix_wins_and_adjacent_groups_merge():
    g = build_param_groups(NAMES, freeze=["unet.encoder"], lr_scale={"unet": 0.5, "unet.encoder.1": 0.25, "unet.decoder": 0.1},
                           weight_decay_scale={"unet.decoder.0.weight": 0.0}, l2_sp=0.01)
    assert g == [(0, 1, 1.0, 1.0, 0.01),          # condition_embed: no prefix matches
                 (2, 3, 0.5, 1.0, 0.01),          # unet.*: merged
                 (4, 5, 0.0, 1.0, 0.0),           # unet.encoder frozen (longer than "unet"); a frozen tensor carries no pull
                 (6, 6, 0.25, 1.0, 0.01),         # unet.encoder.1: the longest prefix wins over freeze's unet.encoder
                 (7, 7, 0.5, 1.0, 0.01),          # unet.encoder2 is not under the prefix unet.encoder
                 (8, 8, 0.1, 0.0, 0.01),
                 (9, 9, 0.5, 1.0, 0.01)]
    assert g[0][0] == 0 and g[-1][1] == len(NAMES) - 1 and all(a[1] + 1 == b[0] for a, b in zip(g, g[1:]))      # covers every parameter
    assert build_param_groups(NAMES) == [(0, len(NAMES) - 1, 1.0, 1.0, 0.0)]
    assert merge_param_groups([(0, 0, 1, 1, 0), (1, 3, 1.0, 1.0, 0.0), (4, 4, 0, 1, 0)], 5) == [(0, 3, 1.0, 1.0, 0.0), (4, 4, 0.0, 1.0, 0.0)]


def test_builder_errors():
    with pytest.raises(ValueError, match="matches no parameter"):
        build_param_groups(NAMES, freeze=["unet.enc"])              # a string prefix, not a name prefix
    with pytest.raises(ValueError, match="matches no parameter"):
        build_param_groups(NAMES, weight_decay_scale={"vae": 0.0})
    with pytest.raises(ValueError, match="both freeze and lr_scale"):
        build_param_groups(NAMES, freeze=["unet.encoder"], lr_scale={"unet.encoder": 0.1})
    # a module without parameters (this model's unet.time_embed) is accepted when the caller names the modules, and selects nothing
    assert build_param_groups(NAMES, freeze=["unet.time_embed"], module_names=["unet", "unet.time_embed"]) == build_param_groups(NAMES)
    with pytest.raises(ValueError, match="matches no parameter"):
        build_param_groups(NAMES, freeze=["unet.time_embed"])
    with pytest.raises(ValueError):
        build_param_groups(NAMES, lr_scale={"unet": -1.0})
    for bad in ([(1, 4, 1, 1, 0)], [(0, 2, 1, 1, 0), (2, 4, 1, 1, 0)], [(0, 3, 1, 1, 0)], [(0, 4, 1, float("nan"), 0)]):
        with pytest.raises(ValueError):
            merge_param_groups(bad, 5)


# ---- load_pretrained ------------------------------------------------------------------------------------------------------------------
def small(seed, **diffusion):
    conf = config(SM_H, T=50, p=0.0)
    conf["model"]["diffusion"].update(diffusion)
    torch.manual_seed(seed)
    m = BiologyAwareDiffusionModel(config=conf, **SM)
    for k, v in diffusion.items():
        setattr(m, k, v)
    return m, conf


@pytest.fixture(scope="module")
def panels():
    a = TH.panel_a()
    return a, TH.panel_b(a)


@pytest.fixture(scope="module")
def adapted(panels):
    """Source model on panel A, a fresh model on panel B, and the fresh model after load_pretrained: read-only."""
    a, b = panels
    src, conf = small(1)
    fresh, _ = small(2)
    tgt = copy.deepcopy(fresh)
    ckpt = {"model_state_dict": src.state_dict(), "config": conf, "feature_names": a}
    report = load_pretrained(tgt, ckpt, b)
    return src, fresh, tgt, report


def test_load_pretrained_matches_columns_by_name(panels, adapted):
    a, b = panels
    src, fresh, tgt, report = adapted
    ka, kb = TH.flat_names(a), TH.flat_names(b)
    s, f, t = src.state_dict(), fresh.state_dict(), tgt.state_dict()
    new_cols = [i for i, k in enumerate(kb) if k not in ka]
    assert len(new_cols) == 4
    for i, k in enumerate(kb):
        if k in ka:
            j = ka.index(k)
            assert torch.equal(t["unet.input_proj.weight"][:, i], s["unet.input_proj.weight"][:, j])
            assert torch.equal(t["unet.output_proj.weight"][i], s["unet.output_proj.weight"][j])
            assert torch.equal(t["unet.output_proj.bias"][i], s["unet.output_proj.bias"][j])
        else:
            assert not t["unet.input_proj.weight"][:, i].any()                                    # a new input starts with no influence
            assert torch.equal(t["unet.output_proj.weight"][i], f["unet.output_proj.weight"][i])      # a new output keeps the fresh init
            assert torch.equal(t["unet.output_proj.bias"][i], f["unet.output_proj.bias"][i])
            assert f["unet.output_proj.weight"][i].any()
    for i, n in enumerate(b["conditions"]):
        assert torch.equal(t["condition_embed.mlp.0.weight"][:, i], s["condition_embed.mlp.0.weight"][:, a["conditions"].index(n)])
    special = set(report["touched"])
    assert special == {"unet.input_proj.weight", "unet.output_proj.weight", "unet.output_proj.bias", "condition_embed.mlp.0.weight"}
    for name, _ in tgt.named_parameters():
        if name not in special:
            assert torch.equal(t[name], s[name]), name
    for name, buf in tgt.named_buffers():
        assert torch.equal(buf, f[name]), name


def test_load_pretrained_input_proj_in_float64(panels, adapted):
    """input_proj of the adapted model on a B-row equals the source's on the corresponding A-row with the dropped columns at 0: in
    float64 both are sums of the same products (plus exact zeros), so only their order differs -- 40 terms of magnitude <= |w||x|,
    each addition rounding by 2^-53 relative: 40 * 2^-53 * sum|w x| bounds the difference."""
    a, b = panels
    src, _, tgt, _ = adapted
    ka, kb = TH.flat_names(a), TH.flat_names(b)
    gen = torch.Generator().manual_seed(0)
    xb = torch.randn(5, len(kb), generator=gen, dtype=torch.float64)
    xa = torch.zeros(5, len(ka), dtype=torch.float64)
    for i, k in enumerate(kb):
        if k in ka:
            xa[:, ka.index(k)] = xb[:, i]
    dropped = [j for j, k in enumerate(ka) if k not in kb]
    assert len(dropped) == 4 and not xa[:, dropped].any()
    ws, bs = src.unet.input_proj.weight.double(), src.unet.input_proj.bias.double()
    wt, bt = tgt.unet.input_proj.weight.double(), tgt.unet.input_proj.bias.double()
    ya, yb = xa @ ws.T + bs, xb @ wt.T + bt
    bound = 40 * 2.0 ** -53 * (xa.abs() @ ws.abs().T + bs.abs())
    assert (ya - yb).abs().le(bound).all() and ya.abs().max() > 0.1


def test_load_pretrained_report(panels, adapted):
    a, b = panels
    _, _, tgt, report = adapted
    assert report["positional"] is False
    assert report["counts"]["expression"] == {"matched": 20, "source_only": 4, "target_only": 4}
    assert report["counts"]["mutations"] == {"matched": 8, "source_only": 0, "target_only": 0}
    assert report["counts"]["pathways"] == {"matched": 8, "source_only": 0, "target_only": 0}
    assert report["counts"]["conditions"] == {"matched": 3, "source_only": 0, "target_only": 0}
    assert report["expression"]["source_only"] == [f"GENE{i}" for i in range(4)]
    assert sorted(report["expression"]["target_only"]) == [f"NEW{i}" for i in range(4)]
    mask = report["mask"]
    total = sum(p.numel() for p in tgt.parameters())
    assert mask.dtype == torch.bool and mask.shape == (total,)
    h0 = SM_H[0]
    assert int((~mask).sum()) == 4 * h0 + 4 * tgt.unet.output_proj.weight.shape[1] + 4      # 4 input columns, 4 output rows, 4 biases
    # the mask follows named_parameters() order: the input_proj slice has exactly the new columns cleared
    off = 0
    for name, p in tgt.named_parameters():
        if name == "unet.input_proj.weight":
            m = mask[off:off + p.numel()].view_as(p)
            new = [i for i, k in enumerate(TH.flat_names(b)) if k[1].startswith("NEW")]
            assert not m[:, new].any() and int(m.sum()) == p.numel() - 4 * h0
        off += p.numel()


def test_load_pretrained_name_sources(panels, tmp_path, caplog):
    a, b = panels
    src, conf = small(1)
    base = {"model_state_dict": src.state_dict(), "config": conf}
    want, _ = small(2)
    load_pretrained(want, dict(base, feature_names=a), b)
    # source_features as a mapping and as a JSON path; it takes precedence over the checkpoint's own names
    for sf in (a, tmp_path / "a.json"):
        if not isinstance(sf, dict):
            sf.write_text(json.dumps(a))
        got, _ = small(2)
        load_pretrained(got, dict(base, feature_names=b), b, source_features=sf)
        assert all(torch.equal(v, want.state_dict()[k]) for k, v in got.state_dict().items())
    # neither, equal widths: positional, with a warning
    got, _ = small(2)
    with caplog.at_level(logging.WARNING, logger="osteosarcoma_diffusionmodel_amd.transfer"):
        rep = load_pretrained(got, base, b)
    assert rep["positional"] and "position" in caplog.text and bool(rep["mask"].all())
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in got.state_dict().items())
    # use_ema: the averaged weights when the file has them, the last iterate on request
    ema_sd = {k: v + 1.0 if k.startswith(("unet", "condition_embed")) else v for k, v in src.state_dict().items()}
    with_ema = dict(base, feature_names=a, ema_state_dict=dict(ema_sd, decay=0.99, warmup=True, num_updates=3))
    got, _ = small(2)
    load_pretrained(got, with_ema, a)
    assert torch.equal(got.state_dict()["unet.encoder.0.0.weight"], ema_sd["unet.encoder.0.0.weight"])
    load_pretrained(got, with_ema, a, use_ema=False)
    assert torch.equal(got.state_dict()["unet.encoder.0.0.weight"], src.state_dict()["unet.encoder.0.0.weight"])
    with pytest.raises(KeyError):
        load_pretrained(got, dict(base, feature_names=a), a, use_ema=True)


def test_load_pretrained_errors(panels):
    a, b = panels
    src, conf = small(1)
    base = {"model_state_dict": src.state_dict(), "config": conf, "feature_names": a}

    def fresh(**kw):
        return small(2, **kw)[0]

    # neither source of names and differing widths
    wide = copy.deepcopy(b)
    wide["expression"] = wide["expression"] + ["EXTRA"]
    torch.manual_seed(0)
    m_wide = BiologyAwareDiffusionModel(config=config(SM_H, T=50, p=0.0), **dict(SM, expression_dim=25))
    with pytest.raises(ValueError, match="which are which"):
        load_pretrained(m_wide, {k: v for k, v in base.items() if k != "feature_names"}, wide)
    load_pretrained(m_wide, base, wide)                       # with names the wider panel is fine
    # hidden widths
    torch.manual_seed(0)
    other = BiologyAwareDiffusionModel(config=config([32, 64, 64], T=50, p=0.0), **SM)
    with pytest.raises(ValueError, match=r"unet\.(encoder|decoder)"):
        load_pretrained(other, base, b)
    # prediction_type, mutation_link, feature_transform
    with pytest.raises(ValueError, match="prediction_type"):
        load_pretrained(fresh(prediction_type="v"), base, b)
    conf_link = copy.deepcopy(conf)
    conf_link["model"]["diffusion"]["mutation_link"] = "logistic"
    with pytest.raises(ValueError, match="mutation_link"):
        load_pretrained(fresh(), dict(base, config=conf_link), b)
    with pytest.raises(ValueError, match="feature_transform"):
        load_pretrained(fresh(), dict(base, feature_transform={}), b)
    # names that do not fit the weights they describe
    with pytest.raises(ValueError):
        load_pretrained(fresh(), base, dict(b, expression=b["expression"][:-1]))
    with pytest.raises(ValueError):
        load_pretrained(fresh(), dict(base, feature_names=dict(a, mutations=a["mutations"][:-1])), b)
    with pytest.raises(ValueError, match="duplicate"):
        load_pretrained(fresh(), base, dict(b, pathways=[b["pathways"][0]] * 8))
    # nothing was written by a refused call
    m = fresh()
    before = copy.deepcopy(m.state_dict())
    with pytest.raises(ValueError):
        load_pretrained(m, dict(base, config=conf_link), b)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


# ---- the restatement against torch.optim.AdamW ----------------------------------------------------------------------------------------
def test_group_adamw_ref_one_default_group_against_torch():
    """5 steps, clipped and unclipped alternating, against clip_grad_norm_ + torch.optim.AdamW on CPU float32.

    Both sides round to float32 (u = 2^-24) and use the same float32 constants; they may differ in how an expression is grouped or
    fused: lerp and addcmul / addcdiv with or without an FMA, value * (a / b) or (value * a) / b.  coef is taken from the norm
    clip_grad_norm_ returns, and torch forms max_norm / (norm + 1e-6), the clamp and g * coef in float32 as the kernel does, so the
    clipped gradient must be EQUAL.  For the rest the bound is a running error budget from the operation count, evaluated with the
    magnitudes of the restatement's own operands (never with a difference between the two sides):
      m = m + w (g - m): 3 operations, each result at most |g| + |m_prev| in magnitude:     E_m += 3 u (|g| + |m_prev|)
      v = v b2 + ((1 - b2) g) g: 4 operations on non-negative terms, each at most v_new:       E_v += 4 u v_new
      upd = nss * (m / denom), denom = sqrt(v) / bc2_sqrt + eps: E_m enters as |nss| E_m / denom, E_v through the square root at half its
        relative size, and sqrt, the two divisions, the add and the scale round once each (5 u, 6 u with one regrouping):
                                                                            E_upd = |nss| E_m / denom + |upd| (E_v / (2 v) + 6 u)
      p = p decay + upd: the product is the same operation on both sides (u |p| only through E_p, which a factor decay < 1 carries), the
        sum rounds once:                                                   E_p = E_p + E_upd + u |p_new|
    with a factor 2 over the first-order budget for the products of errors it leaves out."""
    n, lr, b1, b2, eps, wd, max_norm = 4099, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0
    gen = torch.Generator().manual_seed(0)
    p_t = torch.nn.Parameter(torch.randn(n, generator=gen))
    opt = torch.optim.AdamW([p_t], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p_t.detach().numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    u = 2.0 ** -24
    E_m, E_v, E_p = np.zeros(n), np.zeros(n), np.zeros(n)
    grp = (0, n, 1.0, 1.0, 0.0)
    for step in range(1, 6):
        g = (torch.randn(n, generator=gen) * (10.0 if step % 2 else 0.001)).numpy()
        p_t.grad = torch.from_numpy(g.copy())
        norm = torch.nn.utils.clip_grad_norm_([p_t], max_norm)
        opt.step()
        coef = TH.clip_coef(norm.numpy(), max_norm)
        assert (coef < 1.0) == bool(step % 2)
        m_prev = np.abs(m).astype(np.float64)
        p, g_out, m, v, _ = TH.group_adamw_ref(p, g, m, v, None, None, [grp], lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd,
                                               max_norm=max_norm, step=step, ema_decay=0.0, coef=coef)
        assert np.array_equal(g_out, p_t.grad.numpy()), f"step {step}: the clipped gradient"
        _, nss, _ = TH.group_consts(grp, lr, b1, wd, step)
        bc2s, eps32 = TH.shared_consts(b1, b2, eps, step)[3:]
        m64, v64 = m.astype(np.float64), v.astype(np.float64)
        denom = np.sqrt(v64) / bc2s + eps32
        upd = np.abs(float(nss) * m64 / denom)
        E_m = E_m + 3 * u * (np.abs(g_out) + m_prev)
        E_v = E_v + 4 * u * v64
        E_p = E_p + abs(float(nss)) * E_m / denom + upd * (E_v / (2 * v64) + 6 * u) + u * np.abs(p)
        st = opt.state[p_t]
        for name, got, want, budget in (("exp_avg", m, st["exp_avg"], E_m), ("exp_avg_sq", v, st["exp_avg_sq"], E_v), ("param", p, p_t.detach(), E_p)):
            err = np.abs(got.astype(np.float64) - want.numpy().astype(np.float64))
            assert np.all(err <= 2 * budget), f"step {step}: {name} off by up to {(err / budget).max():.2f} budgets"
    assert float(np.abs(p - p_t.detach().numpy()).max()) <= 1e-6       # the budget itself is tight: a few ulps of |p| ~ 1 after 5 steps
    assert float((2 * E_p).max()) < 1e-5


def test_group_adamw_ref_leaves_frozen_groups_alone():
    n = 64
    rng = np.random.default_rng(0)
    p, g, m, v, e, a = (rng.standard_normal(n).astype(np.float32) for _ in range(6))
    g[:16] = np.nan
    groups = [(0, 16, 0.0, 1.0, 0.5), (16, 40, 0.1, 1.0, 0.0), (40, 64, 1.0, 0.0, 0.5)]
    out = TH.group_adamw_ref(p, g, m, np.abs(v), e, a, groups, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, max_norm=1.0,
                             step=1, ema_decay=0.5, coef=0.5)
    for got, was in zip(out, (p, g, m, np.abs(v), e)):
        assert np.array_equal(got[:16], was[:16], equal_nan=True) and np.isfinite(got[16:]).all() and not np.array_equal(got[16:], was[16:])
    # the pull moves p toward the anchor: with lr_scale 1 and no decay, against the same step without it
    no_pull = TH.group_adamw_ref(p, g, m, np.abs(v), e, a, [(0, 16, 0.0, 1.0, 0.0), (16, 40, 0.1, 1.0, 0.0), (40, 64, 1.0, 0.0, 0.0)], lr=1e-3,
                                 beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, max_norm=1.0, step=1, ema_decay=0.5, coef=0.5)
    d = (out[0] - no_pull[0])[40:].astype(np.float64)
    want = -(1e-3 * 0.5) * (p[40:].astype(np.float64) - a[40:])
    assert np.allclose(d, want, rtol=0, atol=4 * 2.0 ** -24 * np.abs(p[40:]).max())
    assert np.array_equal(out[0][16:40], no_pull[0][16:40])


# ---- argument checks of the two entry points ------------------------------------------------------------------------------------------
def _call(variant, *, bufs=None, null=None, n=100, groups=((0, 100, 1.0, 1.0, 0.0),), n_groups=None, ema=False, anchor=False, ema_decay=0.5,
          step=1, handle=True):
    """Calls one of the two entry points with host arrays standing in for device buffers: every case here must be refused before any
    device call, hence before any of them (or the stand-in handle) is touched."""
    arrs = {k: np.zeros(128, np.float32) for k in ("param", "grad", "exp_avg", "exp_avg_sq", "ema", "anchor")}
    ws = np.zeros(L.OSD_GROUP_WS_DOUBLES, np.float64)
    fake_handle = np.zeros(8192, np.uint8)
    ptr = {k: TH.host_ptr(a) for k, a in arrs.items()}
    if not ema:
        ptr["ema"] = None
    if not anchor:
        ptr["anchor"] = None
    for k in (null or ()):
        ptr[k] = None
    tab = TH.group_table(L, list(groups)) if groups is not None else None
    ng = len(groups) if n_groups is None else n_groups
    tail = (ptr["param"], ptr["grad"], ptr["exp_avg"], ptr["exp_avg_sq"], ptr["ema"], ptr["anchor"], n, tab, ng, 1e-3, 0.9, 0.999, 1e-8, 1e-2,
            1.0, step, ema_decay, None)
    if variant == "handle":
        rc = L.lib().osd_group_adamw_step(TH.host_ptr(fake_handle) if handle else None, *tail)
    else:
        rc = L.lib().osd_nn_group_adamw_step(None, 0, None if "ws" in (null or ()) else TH.host_ptr(ws), *tail)
    return rc, L.last_error()


@pytest.mark.parametrize("variant", ["handle", "nn"])
def test_entry_points_reject_bad_arguments_before_the_device(variant):
    bad = [
        (dict(null=["param"]), "null"), (dict(null=["grad"]), "null"), (dict(null=["exp_avg"]), "null"), (dict(null=["exp_avg_sq"]), "null"),
        (dict(groups=None, n_groups=1), "null"),
        (dict(n_groups=0), "n_groups"), (dict(n_groups=1025), "n_groups"), (dict(n_groups=-3), "n_groups"),
        (dict(groups=[(0, 60, 1, 1, 0), (50, 100, 1, 1, 0)]), "group 1"),            # overlapping
        (dict(groups=[(50, 100, 1, 1, 0), (0, 50, 1, 1, 0)]), "group 0"),            # unsorted
        (dict(groups=[(0, 50, 1, 1, 0), (50, 50, 1, 1, 0), (50, 100, 1, 1, 0)]), "group 1"),      # empty
        (dict(groups=[(0, 50, 1, 1, 0), (60, 100, 1, 1, 0)]), "group 1"),            # a gap
        (dict(groups=[(0, 50, 1, 1, 0), (50, 90, 1, 1, 0)]), "numel"),               # stops short of numel
        (dict(groups=[(0, 50, 1, 1, 0), (50, 101, 1, 1, 0)]), "group 1"),            # past numel
        (dict(groups=[(1, 100, 1, 1, 0)]), "group 0"),                               # does not start at 0
        (dict(groups=[(0, 100, -0.5, 1, 0)]), ">= 0"), (dict(groups=[(0, 100, 1, float("nan"), 0)]), ">= 0"),
        (dict(groups=[(0, 100, 1, 1, float("inf"))], anchor=True), ">= 0"), (dict(groups=[(0, 100, 1, -1.0, 0)]), ">= 0"),
        (dict(groups=[(0, 50, 1, 1, 0), (50, 100, 1, 1, 0.5)]), "anchor"),           # l2sp > 0 with a null anchor
        (dict(ema=True, ema_decay=1.5), "ema_decay"), (dict(ema=True, ema_decay=-0.1), "ema_decay"), (dict(ema=True, ema_decay=float("nan")), "ema_decay"),
        (dict(n=0, groups=[(0, 100, 1, 1, 0)]), "positive"), (dict(step=0), "positive"),
    ]
    if variant == "handle":
        bad.append((dict(handle=False), "null"))
    else:
        bad.append((dict(null=["ws"]), "null"))
    for kw, word in bad:
        rc, msg = _call(variant, **kw)
        assert rc == L.OSD_EINVAL, (kw, rc, msg)
        assert word in msg, (kw, msg)
    # a well-formed call gets past the checks and fails at the first device call instead: there is no device
    rc, msg = _call(variant, groups=[(0, 50, 0.0, 1, 0), (50, 100, 1, 1, 0.5)], anchor=True, ema=True)
    assert rc == L.OSD_EHIP, (rc, msg)
    assert C.sizeof(L.OsdParamGroup) == 32


# ---- Trainer refusals -----------------------------------------------------------------------------------------------------------------
def train_conf(save_dir, **extra):
    conf = config(SM_H, T=50, p=0.0)
    conf["training"] = {"learning_rate": 3e-3, "weight_decay": 1e-5, "patience": 100, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.0},
                        "save_dir": str(save_dir), "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": 16,
                        **extra}
    return conf


def test_trainer_refusals_come_before_the_device(tmp_path):
    """device="cuda" on a machine without one: anything but the expected ValueError would be a RuntimeError from the runtime."""
    def trainer(model=None, **extra):
        conf = train_conf(tmp_path, **extra)
        torch.manual_seed(0)
        return Trainer(model if model is not None else BiologyAwareDiffusionModel(config=conf, **SM), [], [], conf, device="cuda")

    with pytest.raises(ValueError, match="training.dp"):
        trainer(finetune={}, dp={"max_grad_norm": 1.0, "noise_multiplier": 1.0})
    vae_conf = {"model": {"latent_dim": 16, "hidden_dims": [32, 64, 32], "gnn": {"dropout": 0.2},
                          "constraints": {"pathway_coherence_weight": 1.0, "mutation_expression_weight": 0.5, "survival_prediction_weight": 0.3}}}
    with pytest.raises(ValueError, match="cVAE"):
        trainer(model=BiologyConstrainedVAE(8, 24, 8, 3, vae_conf), finetune={})
    with pytest.raises(ValueError, match="matches no parameter"):
        trainer(finetune={"freeze": ["unet.nothing"]})
    with pytest.raises(ValueError, match="both freeze and lr_scale"):
        trainer(finetune={"freeze": ["unet.encoder"], "lr_scale": {"unet.encoder": 0.5}})
    with pytest.raises(ValueError, match="unknown keys"):
        trainer(finetune={"freze": []})
    with pytest.raises(ValueError, match="save_feature_names"):
        trainer(save_feature_names=True)
    torch.distributed.init_process_group("gloo", store=torch.distributed.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        with pytest.raises(ValueError, match="torch.distributed"):
            trainer(finetune={})
    finally:
        torch.distributed.destroy_process_group()
