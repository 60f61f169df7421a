"""Carry a pretrained diffusion checkpoint onto a model with another feature panel.

Another cohort's top-variance genes are not the same columns, so three tensors of the denoiser cannot be copied as they are: the ones
that touch raw columns.  ``load_pretrained`` matches their columns by (block, name) and copies every other tensor whole:

* ``unet.input_proj.weight`` (hidden x D): matched columns are copied; a column the source lacks is set to ZERO, so a new input starts
  with no influence on the trunk the other weights were trained for;
* ``unet.output_proj.weight`` / ``.bias`` (D rows): matched rows are copied; a row the source lacks keeps the model's own fresh
  initialisation (a zero row would start with a zero gradient path into nothing but the bias);
* ``condition_embed.mlp.0.weight`` (64 x conditions): columns matched by condition name; unmatched columns are set to zero.

A shape mismatch anywhere else -- hidden widths, the time dimension -- and a checkpoint trained with another ``prediction_type`` or
``mutation_link``, or behind a ``feature_transform``, is a ValueError naming what differs."""
from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Dict, List, Optional, Union

import torch
import torch.nn as nn

logger = logging.getLogger(__name__)

BLOCKS = ("mutations", "expression", "pathways")
INPUT_W, OUTPUT_W, OUTPUT_B, COND_W = ("unet.input_proj.weight", "unet.output_proj.weight", "unet.output_proj.bias",
                                       "condition_embed.mlp.0.weight")


def check_feature_names(fn, what: str) -> Dict[str, List[str]]:
    """A ``feature_names`` mapping: the three data blocks and ``conditions``, each a list of distinct strings."""
    if not isinstance(fn, dict) or any(k not in fn for k in BLOCKS + ("conditions",)):
        raise ValueError(f"{what} must map {BLOCKS + ('conditions',)} to lists of names")
    out = {}
    for k in BLOCKS + ("conditions",):
        names = [str(n) for n in fn[k]]
        if len(set(names)) != len(names):
            raise ValueError(f"{what}[{k!r}] holds duplicate names")
        out[k] = names
    return out


def _column_keys(fn: Dict[str, List[str]]) -> List[tuple]:
    return [(blk, n) for blk in BLOCKS for n in fn[blk]]


def _source_features(checkpoint: dict, source_features) -> Optional[Dict[str, List[str]]]:
    if source_features is not None:
        if isinstance(source_features, (str, Path)):
            source_features = json.loads(Path(source_features).read_text())
        return check_feature_names(source_features, "source_features")
    if checkpoint.get("feature_names") is not None:
        return check_feature_names(checkpoint["feature_names"], "the checkpoint's feature_names")
    return None


def _check_compatible(model: nn.Module, checkpoint: dict):
    if "feature_transform" in checkpoint:
        raise ValueError("the checkpoint was trained behind a data.transform (feature_transform): its quantile tables belong to the source "
                         "panel's columns and cannot be carried onto another panel")
    dm = ((checkpoint.get("config") or {}).get("model") or {}).get("diffusion") or {}
    for key, default in (("prediction_type", "epsilon"), ("mutation_link", "identity")):
        saved, own = dm.get(key) or default, getattr(model, key, None) or default
        if saved != own:
            raise ValueError(f"{key}: the checkpoint was trained with {saved!r}, the model has {own!r}")


def load_pretrained(model: nn.Module, checkpoint_or_path: Union[dict, str, Path], feature_names, source_features=None,
                    use_ema: Optional[bool] = None) -> dict:
    """Copy a diffusion checkpoint into ``model`` in place (see the module docstring for the three tensors matched by column name).

    ``feature_names``: the model's own panel, ``{"mutations": [...], "expression": [...], "pathways": [...], "conditions": [...]}``
    (None: unknown, which leaves only the positional case below).
    The source's names come from ``source_features`` (such a mapping, or the path of a JSON file holding one), else from the checkpoint's
    ``feature_names`` (``training.save_feature_names``); with neither and equal widths the columns are taken by position, with a logged
    warning; with neither and differing widths it is a ValueError.  ``use_ema``: as in ``load_trained_model`` (None: the averaged
    weights when the file has them).

    Returns a report: per block (and ``conditions``) ``{"matched", "source_only", "target_only"}`` name lists and ``counts``; ``touched``,
    the parameter names whose columns were matched rather than copied whole; ``positional``; and ``mask``, a flat bool tensor in
    ``named_parameters()`` order (``FlatParams``' layout), True where the element came from the checkpoint."""
    if hasattr(model, "vae"):
        raise ValueError("load_pretrained carries a diffusion checkpoint; a cVAE model is not accepted")
    ckpt = checkpoint_or_path
    if isinstance(ckpt, (str, Path)):
        ckpt = torch.load(ckpt, map_location="cpu", weights_only=True)
    has_ema = "ema_state_dict" in ckpt
    if use_ema and not has_ema:
        raise KeyError("use_ema=True but the checkpoint has no ema_state_dict (train with training.ema_decay)")
    if has_ema and (use_ema is None or use_ema):
        from .train import ParamEMA
        src = ParamEMA.model_state(ckpt["ema_state_dict"])
    else:
        src = ckpt["model_state_dict"]
    _check_compatible(model, ckpt)
    params = dict(model.named_parameters())
    for name in (INPUT_W, OUTPUT_W, OUTPUT_B, COND_W):
        if name not in params or name not in src:
            raise ValueError(f"{name} is missing from the {'model' if name not in params else 'checkpoint'}: not a diffusion denoiser")
    D = params[INPUT_W].shape[1]
    widths = [getattr(model, a) for a in ("mutation_dim", "expression_dim", "pathway_dim")]
    names_src = _source_features(ckpt, source_features)
    if feature_names is None:
        # no names for the model's own panel: nothing can be matched by name, so the source's names are not used either
        names_src = None
        own = {**{b: [f"{b}:{i}" for i in range(w)] for b, w in zip(BLOCKS, widths)},
               "conditions": [f"condition:{i}" for i in range(params[COND_W].shape[1])]}
    else:
        own = check_feature_names(feature_names, "feature_names")
    if [len(own[b]) for b in BLOCKS] != widths or len(own["conditions"]) != params[COND_W].shape[1]:
        raise ValueError(f"feature_names has {[len(own[b]) for b in BLOCKS]} data columns and {len(own['conditions'])} conditions, the model "
                         f"{widths} and {params[COND_W].shape[1]}")
    src_D, src_C = src[INPUT_W].shape[1], src[COND_W].shape[1]
    positional = names_src is None
    if positional:
        if src_D != D or src_C != params[COND_W].shape[1]:
            raise ValueError(f"the checkpoint has {src_D} data columns and {src_C} conditions, the model {D} and {params[COND_W].shape[1]}, and "
                             "no feature names on both sides (feature_names; source_features or the checkpoint's feature_names) say which are which")
        logger.warning("load_pretrained: no feature names on both sides (feature_names; source_features or the checkpoint's feature_names): "
                       "columns are taken by position")
        names_src = own
    if len(_column_keys(names_src)) != src_D or len(names_src["conditions"]) != src_C:
        raise ValueError(f"the source's feature names list {len(_column_keys(names_src))} data columns and {len(names_src['conditions'])} "
                         f"conditions, its weights have {src_D} and {src_C}")
    if src[OUTPUT_W].shape[0] != src_D or src[OUTPUT_B].shape[0] != src_D:
        raise ValueError(f"{OUTPUT_W}: the checkpoint's output_proj has {src[OUTPUT_W].shape[0]} rows for {src_D} input columns")

    def match(own_keys, src_keys):
        where = {k: j for j, k in enumerate(src_keys)}
        pairs = [(i, where[k]) for i, k in enumerate(own_keys) if k in where]
        own_idx = torch.tensor([i for i, _ in pairs], dtype=torch.int64)
        src_idx = torch.tensor([j for _, j in pairs], dtype=torch.int64)
        return own_idx, src_idx

    col_own, col_src = match(_column_keys(own), _column_keys(names_src))
    cond_own, cond_src = match(own["conditions"], names_src["conditions"])
    special = {INPUT_W, OUTPUT_W, OUTPUT_B, COND_W}
    for name, p in params.items():                # every check before the first write
        if name not in src:
            raise ValueError(f"{name} is missing from the checkpoint")
        want = tuple(p.shape)
        got = tuple(src[name].shape)
        if name in (INPUT_W, COND_W):
            ok = got[0] == want[0]
        elif name == OUTPUT_W:
            ok = got[1] == want[1]
        elif name == OUTPUT_B:
            ok = True
        else:
            ok = got == want
        if not ok:
            raise ValueError(f"{name}: the checkpoint has shape {got}, the model {want}")
    masks = {}
    with torch.no_grad():
        for name, p in params.items():
            s = src[name].to(device=p.device, dtype=p.dtype)
            mask = torch.zeros(p.shape, dtype=torch.bool)
            if name == INPUT_W:
                p.zero_()
                p[:, col_own.to(p.device)] = s[:, col_src.to(p.device)]
                mask[:, col_own] = True
            elif name == COND_W:
                p.zero_()
                p[:, cond_own.to(p.device)] = s[:, cond_src.to(p.device)]
                mask[:, cond_own] = True
            elif name in (OUTPUT_W, OUTPUT_B):
                p[col_own.to(p.device)] = s[col_src.to(p.device)]
                mask[col_own] = True
            else:
                p.copy_(s)
                mask[...] = True
            masks[name] = mask
    # buffers (the noise schedule's tables) stay the model's own: they follow its config, not the source run's
    for e in getattr(model, "_engines", {}).values():      # an engine that already packed the old weights re-derives its tables
        e._sig = None
    report = {"positional": positional, "touched": sorted(special), "counts": {}}
    for blk in BLOCKS + ("conditions",):
        a, b = own[blk], names_src[blk]
        sa, sb = set(a), set(b)
        report[blk] = {"matched": [n for n in a if n in sb], "source_only": [n for n in b if n not in sa], "target_only": [n for n in a if n not in sb]}
        report["counts"][blk] = {k: len(v) for k, v in report[blk].items()}
    report["mask"] = torch.cat([masks[name].reshape(-1) for name in params])
    logger.info("load_pretrained: " + ", ".join(f"{blk} {c['matched']} matched / {c['source_only']} source-only / {c['target_only']} new"
                                                for blk, c in report["counts"].items()))
    return report
