"""Shared by tests/test_transfer_cpu.py and tests/test_gpu_transfer.py: the grouped AdamW step restated in NumPy float32 (one rounding
per operation, as the kernel's __f*_rn chain), group tables, and the two gene panels of the transfer tests."""
import ctypes as C
import math

import numpy as np

F = np.float32


def group_consts(group, lr, beta1, weight_decay, step):
    """(decay_s, neg_step_size_s, pull_s) of one group: formed in double, rounded once to float (include/osdiff.h)."""
    lr_s, wd_s, l2sp = (float(F(x)) for x in group[2:5])        # the C struct holds floats
    bc1 = 1.0 - beta1 ** step
    lr_k = lr * lr_s
    return F(1.0 - lr_k * weight_decay * wd_s), F(-(lr_k / bc1)), F(lr_k * l2sp)


def shared_consts(beta1, beta2, eps, step):
    bc2 = 1.0 - beta2 ** step
    return F(1.0 - beta1), F(beta2), F(1.0 - beta2), F(math.sqrt(bc2)), F(eps)


def clip_coef(norm, max_norm):
    """The kernel's clip factor from the float norm it reports: min(1, max_norm / (norm + 1e-6)) in float32; 1 when clipping is off."""
    if not max_norm > 0.0:
        return F(1.0)
    return min(F(max_norm) / (F(norm) + F(1e-6)), F(1.0))


def group_adamw_ref(p, g, m, v, ema, anchor, groups, *, lr, beta1, beta2, eps, weight_decay, max_norm, step, ema_decay, coef):
    """One grouped step on float32 host arrays; returns new (p, g, m, v, ema) and leaves its inputs alone.  ``groups``: a list of
    (begin, end, lr_scale, wd_scale, l2sp) element ranges.  ``coef`` is an input (the norm's summation order is the kernel's own affair);
    ``ema`` / ``anchor`` may be None.  Frozen groups (lr_scale == 0) come back as they went in."""
    p, g, m, v = (np.array(a, dtype=F, copy=True) for a in (p, g, m, v))
    ema = None if ema is None else np.array(ema, dtype=F, copy=True)
    omb1, b2, omb2, bc2s, eps32 = shared_consts(beta1, beta2, eps, step)
    w = F(1.0 - ema_decay)
    coef = F(coef)
    with np.errstate(all="ignore"):
        for grp in groups:
            b, e = int(grp[0]), int(grp[1])
            if float(grp[2]) == 0.0:
                continue
            decay, nss, pull = group_consts(grp, lr, beta1, weight_decay, step)
            gi = g[b:e]
            if max_norm > 0.0:
                gi = gi * coef
                g[b:e] = gi
            p_old = p[b:e]
            pi = p_old * decay
            if pull != 0.0:
                pi = pi - pull * (p_old - anchor[b:e])
            mi = m[b:e] + omb1 * (gi - m[b:e])
            vi = v[b:e] * b2
            vi = vi + (omb2 * gi) * gi
            denom = np.sqrt(vi) / bc2s + eps32
            pi = pi + nss * (mi / denom)
            p[b:e], m[b:e], v[b:e] = pi, mi, vi
            if ema is not None:
                ema[b:e] = ema[b:e] + w * (pi - ema[b:e])
    for a in (p, g, m, v):
        assert a.dtype == F
    return p, g, m, v, ema


def group_table(L, groups):
    """ctypes array of osd_param_group from (begin, end, lr_scale, wd_scale, l2sp) tuples."""
    tab = (L.OsdParamGroup * len(groups))()
    for k, (b, e, lr_s, wd_s, l2sp) in enumerate(groups):
        tab[k] = L.OsdParamGroup(int(b), int(e), lr_s, wd_s, l2sp)
    return tab


def cut(n, boundaries, settings=((1.0, 1.0, 0.0),)):
    """Groups over [0, n) cut at ``boundaries``, the settings cycling."""
    edges = [0] + [b for b in boundaries if 0 < b < n] + [n]
    return [(edges[k], edges[k + 1]) + tuple(settings[k % len(settings)]) for k in range(len(edges) - 1)]


# ---- two gene panels: B is A permuted, with 4 columns dropped and 4 new ones (per block where the block is wide enough) ----
def panel_a(n_mut=8, n_expr=24, n_path=8):
    return {"mutations": [f"MUT{i}" for i in range(n_mut)], "expression": [f"GENE{i}" for i in range(n_expr)],
            "pathways": [f"PATH{i}" for i in range(n_path)], "conditions": ["survival_time", "event_occurred", "metastasis_at_diagnosis"]}


def panel_b(a, seed=3):
    """Same widths as A.  Expression: GENE0..3 dropped, NEW0..3 added, the rest permuted; mutations and pathways: permuted only;
    conditions: reordered."""
    rng = np.random.default_rng(seed)
    expr = a["expression"][4:] + [f"NEW{i}" for i in range(4)]
    return {"mutations": [a["mutations"][i] for i in rng.permutation(len(a["mutations"]))],
            "expression": [expr[i] for i in rng.permutation(len(expr))],
            "pathways": [a["pathways"][i] for i in rng.permutation(len(a["pathways"]))],
            "conditions": [a["conditions"][i] for i in (2, 0, 1)]}


def flat_names(fn):
    """(block, name) of every data column, in column order."""
    return [(blk, n) for blk in ("mutations", "expression", "pathways") for n in fn[blk]]


def host_ptr(arr):
    return C.c_void_p(arr.ctypes.data)
