"""Feature transforms: per-column maps between data units and the units the model diffuses.

A ``FeatureTransform`` is fitted once on the host (NumPy float64; training cohorts have hundreds to a few thousand rows) and then
applied on the device by ``osd_xf_apply`` (csrc/transform.hip): ``forward`` takes data to model units, ``inverse`` takes samples
back.  Each column has a kind -- ``identity``, ``standard`` (centre and scale) or ``quantile_normal`` (a monotone piecewise-linear
map between the column's quantile knots and a shared table of normal levels; ties go to their mid-rank level, the inverse stays
inside the observed range bit for bit).  The definition, op for op, is the comment block of ``osd_xf_apply`` in include/osdiff.h.
The tables travel in checkpoints as plain tensors (``state_dict`` / ``from_state_dict``; ``torch.load(weights_only=True)``).
"""
from __future__ import annotations

import ctypes as C
from statistics import NormalDist
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

BLOCKS = ("mutations", "expression", "pathways")
KINDS = {"identity": L.OSD_XF_IDENTITY, "standard": L.OSD_XF_STANDARD, "quantile_normal": L.OSD_XF_QUANTILE_NORMAL}
MAX_QUANTILES = L.OSD_XF_MAX_Q
LEVEL_CLIP = 1e-7                  # the outermost levels are the normal quantiles of 1e-7 and 1 - 1e-7: about -5.2 and 5.2


def check_spec(spec) -> Dict[str, str]:
    """``spec`` (block -> kind; a missing block is identity) as a full dict over the three blocks.  ValueError on an unknown block or
    kind and on ``mutations`` anything but identity: the mutation block is 0/1 and is thresholded in model units."""
    if not isinstance(spec, dict):
        raise ValueError(f"data.transform: expected a dict of block -> kind, got {type(spec).__name__}")
    extra = set(spec) - set(BLOCKS)
    if extra:
        raise ValueError(f"data.transform: unknown block(s) {sorted(extra)}; expected any of {list(BLOCKS)}")
    full = {}
    for b in BLOCKS:
        kind = spec.get(b)
        kind = "identity" if kind is None else kind
        if kind not in KINDS:
            raise ValueError(f"data.transform: unknown kind {kind!r} for {b}; expected one of {list(KINDS)}")
        full[b] = kind
    if full["mutations"] != "identity":
        raise ValueError("data.transform: mutations must stay identity (0/1 columns, binarised at 0.5 in model units)")
    return full


def transform_config(config: Optional[dict]) -> Optional[Tuple[Dict[str, str], Optional[int]]]:
    """``config['data']['transform']`` as ``(spec, n_quantiles or None)``; None when the key is absent (the default: nothing changes).
    ``{expression: quantile_normal, pathways: standard, n_quantiles: 1000}``."""
    t = ((config or {}).get("data") or {}).get("transform")
    if t is None:
        return None
    if not isinstance(t, dict):
        raise ValueError(f"data.transform: expected a dict, got {type(t).__name__}")
    t = dict(t)
    nq = t.pop("n_quantiles", None)
    if nq is not None and int(nq) < 2:
        raise ValueError(f"data.transform: n_quantiles={nq} must be at least 2")
    return check_spec(t), None if nq is None else int(nq)


def normal_levels(Q: int) -> np.ndarray:
    """float32 [Q]: the normal quantiles of clip(i / (Q - 1), 1e-7, 1 - 1e-7), antisymmetrised in float64 and rounded once."""
    p = np.clip(np.arange(Q, dtype=np.float64) / (Q - 1), LEVEL_CLIP, 1.0 - LEVEL_CLIP)
    nd = NormalDist()
    z = np.array([nd.inv_cdf(float(v)) for v in p], dtype=np.float64)
    return (0.5 * (z - z[::-1])).astype(np.float32)


def check_transform_training(model, constraints_active: bool) -> None:
    """What cannot train behind a feature transform, each a ValueError naming ``data.transform``: a cVAE model, and the constraint
    losses, whose Pearson terms are not invariant under the map."""
    if hasattr(model, "vae"):
        raise ValueError("data.transform maps the diffusion model's features and is not accepted for a cVAE model")
    if constraints_active:
        raise ValueError("data.transform is not supported with the constraint losses: their Pearson terms are not invariant under "
                         "the map (set their weights to 0 or clear them)")


def training_transform(model_ft: Optional["FeatureTransform"], dataset_ft: Optional["FeatureTransform"],
                       dataset_is_raw: bool) -> Optional["FeatureTransform"]:
    """The transform a Trainer's model carries: the dataset's (``prepare_data`` under ``data.transform``), else the model's own, else
    None.  ValueError, naming ``data.transform``, when the two disagree -- the ``load_trained_model`` rule: the checkpoint would claim
    a map the data did not go through.  ``dataset_is_raw``: the dataset is an ``OsteosarcomaDataset`` that carries no transform, i.e.
    its rows are in data units; a model with a transform is refused on it (a caller who mapped the rows by hand sets
    ``dataset.feature_transform = model.feature_transform``)."""
    if model_ft is not None and dataset_ft is not None and model_ft is not dataset_ft and not model_ft.same_as(dataset_ft):
        raise ValueError("the model carries a feature transform (from its checkpoint) that differs from the dataset's data.transform "
                         f"({model_ft.spec}, {int(model_ft.levels.shape[0])} levels against {dataset_ft.spec}, "
                         f"{int(dataset_ft.levels.shape[0])} levels, or other tables): train on data prepared with the same split and "
                         "data.transform, or clear model.feature_transform")
    if model_ft is not None and dataset_ft is None and dataset_is_raw:
        raise ValueError("the model carries a feature transform but the dataset was prepared without data.transform: its rows are in "
                         "data units (set data.transform, or dataset.feature_transform = model.feature_transform for rows mapped by hand)")
    return dataset_ft if dataset_ft is not None else model_ft


def checkpoint_feature_transform(checkpoint: dict, config: Optional[dict]) -> Optional["FeatureTransform"]:
    """The transform a model built from ``config`` must take over from ``checkpoint``: the checkpoint's, or None when it has none.
    ValueError when ``config`` names a ``data.transform`` whose spec (or ``n_quantiles``) differs from the checkpoint's -- decoding
    with another map gives no other sign."""
    saved = checkpoint.get("feature_transform")
    asked = transform_config(config)
    if saved is None:
        if asked is not None and any(k != "identity" for k in asked[0].values()):
            raise ValueError(f"config['data']['transform'] is {asked[0]} but the checkpoint was trained without data.transform")
        return None
    ft = FeatureTransform.from_state_dict(saved)
    if asked is not None:
        if asked[0] != ft.spec:
            raise ValueError(f"config['data']['transform'] is {asked[0]} but the checkpoint was trained with data.transform {ft.spec}")
        if asked[1] is not None and asked[1] != ft.n_quantiles:
            raise ValueError(f"config['data']['transform'] has n_quantiles={asked[1]} but the checkpoint was trained with "
                             f"n_quantiles={ft.n_quantiles}")
    return ft


class FeatureTransform:
    """Per-column maps of a [mutations | expression | pathways] matrix; see the module docstring.  ``kind`` int32 [D], ``knots``
    float32 [D, Q] (zeros for columns that are not quantile columns), ``levels`` float32 [Q], ``center`` / ``scale`` float32 [D]
    (0 / 1 for columns that are not standard columns): host tensors; a copy per device is made at first use."""

    def __init__(self, kind, knots, levels, center, scale, blocks: Dict[str, int], spec: Dict[str, str], n_quantiles: int):
        self.kind = torch.as_tensor(kind, dtype=torch.int32).contiguous().cpu()
        self.knots = torch.as_tensor(knots, dtype=torch.float32).contiguous().cpu()
        self.levels = torch.as_tensor(levels, dtype=torch.float32).contiguous().cpu()
        self.center = torch.as_tensor(center, dtype=torch.float32).contiguous().cpu()
        self.scale = torch.as_tensor(scale, dtype=torch.float32).contiguous().cpu()
        self.blocks = {b: int(blocks[b]) for b in BLOCKS}
        self.spec = check_spec(spec)
        self.n_quantiles = int(n_quantiles)
        D, Q = self.dim, int(self.levels.shape[0])
        if not 2 <= Q <= MAX_QUANTILES:
            raise ValueError(f"levels: {Q} entries, expected 2 .. {MAX_QUANTILES}")
        if tuple(self.kind.shape) != (D,) or tuple(self.knots.shape) != (D, Q) or tuple(self.center.shape) != (D,) \
                or tuple(self.scale.shape) != (D,):
            raise ValueError(f"feature transform tables do not fit {D} columns and {Q} levels")
        if int(((self.kind < 0) | (self.kind > 2)).sum()):
            raise ValueError("kind must be 0 (identity), 1 (standard) or 2 (quantile_normal)")
        lv = self.levels.numpy()
        if not (np.diff(lv) > 0).all():
            raise ValueError("levels must be strictly increasing in float32")
        if not (np.diff(self.knots.numpy(), axis=1) >= 0).all():
            raise ValueError("knots must be non-decreasing along each column's row")
        self._device_tables: Dict[torch.device, tuple] = {}

    @property
    def dim(self) -> int:
        return sum(self.blocks.values())

    def same_as(self, other: "FeatureTransform") -> bool:
        """The same map: blocks, spec and every table, bit for bit."""
        return (self.blocks == other.blocks and self.spec == other.spec
                and all(a.shape == b.shape and torch.equal(a, b) for a, b in
                        ((getattr(self, n), getattr(other, n)) for n in ("kind", "knots", "levels", "center", "scale"))))

    # -- fit ------------------------------------------------------------------------------------------------------------------
    @classmethod
    def fit(cls, features, blocks: Dict[str, int], spec: Dict[str, str], n_quantiles: int = 1000) -> "FeatureTransform":
        """Fit on the rows of ``features`` ([n, D] array or tensor; ``blocks = {"mutations": md, "expression": ed, "pathways": pd}``,
        md + ed + pd = D), on the host in float64.  Non-finite entries are ignored per column.  ``standard``: the column mean and
        ``std(ddof=1) + 1e-8``.  ``quantile_normal``: Q = min(n_quantiles, fewest finite rows of a quantile column, 1024), at least 2
        and the same for every column; knot i is the quantile at level i / (Q - 1), linear between order statistics -- the position
        i (n - 1) / (Q - 1) split into quotient and remainder in integers, interpolated in float64, rounded once to float32.
        ValueError: a column without a finite value, ``mutations`` not identity, an unknown block or kind, ``n_quantiles`` < 2."""
        spec = check_spec(spec)
        extra = set(blocks) - set(BLOCKS)
        if extra:
            raise ValueError(f"blocks: unknown block(s) {sorted(extra)}; expected {list(BLOCKS)}")
        widths = {b: int(blocks.get(b, 0)) for b in BLOCKS}
        n_quantiles = int(n_quantiles)
        if n_quantiles < 2:
            raise ValueError(f"n_quantiles={n_quantiles} must be at least 2")
        if isinstance(features, torch.Tensor):
            features = features.detach().cpu().numpy()
        x = np.array(features, dtype=np.float64)                    # a copy: non-finite entries become NaN below
        D = sum(widths.values())
        if x.ndim != 2 or x.shape[1] != D or x.shape[0] < 1:
            raise ValueError(f"features: expected [rows >= 1, {D}], got {tuple(x.shape)}")
        x[~np.isfinite(x)] = np.nan
        finite = np.isfinite(x).sum(axis=0)
        kind = np.concatenate([np.full(widths[b], KINDS[spec[b]], dtype=np.int32) for b in BLOCKS])
        mapped = kind != L.OSD_XF_IDENTITY
        if (finite[mapped] < 1).any():
            bad = int(np.flatnonzero(mapped & (finite < 1))[0])
            raise ValueError(f"features: column {bad} has no finite value to fit a transform on")

        center, scale = np.zeros(D, dtype=np.float64), np.ones(D, dtype=np.float64)
        std_cols = np.flatnonzero(kind == L.OSD_XF_STANDARD)
        if std_cols.size:
            xs = x[:, std_cols]
            n = finite[std_cols].astype(np.float64)
            mean = np.nansum(xs, axis=0) / n
            ss = np.nansum((xs - mean) ** 2, axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                std = np.where(n > 1, np.sqrt(ss / (n - 1)), 0.0)   # one finite row: no spread to speak of
            center[std_cols], scale[std_cols] = mean, std + 1e-8

        q_cols = np.flatnonzero(kind == L.OSD_XF_QUANTILE_NORMAL)
        Q = max(2, min(n_quantiles, int(finite[q_cols].min()) if q_cols.size else n_quantiles, MAX_QUANTILES))
        knots = np.zeros((D, Q), dtype=np.float32)
        if q_cols.size:
            s = np.sort(x[:, q_cols], axis=0)                       # NaN sorts last: the first n_f rows of a column are its finite values
            n_f = finite[q_cols].astype(np.int64)
            num = np.arange(Q, dtype=np.int64)[:, None] * (n_f - 1)[None, :]        # [Q, columns]
            quot, rem = num // (Q - 1), num % (Q - 1)
            lo = np.take_along_axis(s, quot, axis=0)
            hi = np.take_along_axis(s, np.minimum(quot + 1, (n_f - 1)[None, :]), axis=0)
            knots[q_cols] = (lo + (hi - lo) * (rem.astype(np.float64) / (Q - 1))).astype(np.float32).T
            # rounding to float32 keeps the order of the float64 quantiles
            assert (np.diff(knots[q_cols], axis=1) >= 0).all()
        levels = normal_levels(Q)
        assert (np.diff(levels) > 0).all(), "the levels must be strictly increasing in float32"
        return cls(kind, knots, levels, center.astype(np.float32), scale.astype(np.float32), widths, spec, n_quantiles)

    # -- device maps ----------------------------------------------------------------------------------------------------------
    def _tables(self, device: torch.device) -> tuple:
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device_tables:
            self._device_tables[device] = tuple(t.to(device) for t in (self.kind, self.knots, self.levels, self.center, self.scale))
        return self._device_tables[device]

    def _apply(self, x: torch.Tensor, out: Optional[torch.Tensor], inverse: bool) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected a [rows, {self.dim}] tensor, got {tuple(getattr(x, 'shape', ()))}")
        if not x.is_cuda or (out is not None and not out.is_cuda):
            raise RuntimeError("feature transforms run on a ROCm device: pass device tensors (there is no CPU fallback)")
        D = self.dim

        def rows_ok(t):
            return t.dtype == torch.float32 and t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= D)

        if out is not None and (out.shape != x.shape or out.device != x.device or not rows_ok(out)):
            raise ValueError("out must be a float32 tensor of x's shape on x's device with contiguous rows")
        if not rows_ok(x):
            x = x.to(torch.float32).contiguous()
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        rows = int(x.shape[0])
        if rows == 0:
            return out
        kind, knots, levels, center, scale = self._tables(x.device)
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        index = x.device.index if x.device.index is not None else torch.cuda.current_device()
        L.check(L.lib().osd_xf_apply(stream, index, L.ptr(x), max(int(x.stride(0)), D), L.ptr(out), max(int(out.stride(0)), D), rows, D,
                                     L.ptr(kind), L.ptr(knots), int(levels.shape[0]), L.ptr(levels), L.ptr(center), L.ptr(scale),
                                     1 if inverse else 0))
        return out

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Data units -> model units on the device: ``x`` a float32 device tensor [rows, D] (a row stride, i.e. a column slice of a
        wider matrix, is read in place); ``out`` likewise, ``out=x`` maps in place, None allocates.  NaN stays NaN."""
        return self._apply(x, out, False)

    def inverse(self, z: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Model units -> data units, as ``forward``.  A quantile column's values come back inside its observed range [k[0], k[Q-1]]."""
        return self._apply(z, out, True)

    # -- bounds ---------------------------------------------------------------------------------------------------------------
    def forward_host(self, values) -> np.ndarray:
        """The forward map of ONE value per column, float32 [D] -> float32 [D], on the host: the kernel's rule in NumPy float32, op
        for op (IEEE operations, no contraction), for the 2 x D numbers of ``map_bounds`` -- not a path for data.  A restatement of
        csrc/transform.hip, its bracket clamp (``xf_lerp``) included, which tests/test_gpu_transform.py holds bit-equal to the kernel:
        change the two together."""
        v = np.asarray(values, dtype=np.float32)
        if v.shape != (self.dim,):
            raise ValueError(f"expected [{self.dim}] values, got {tuple(v.shape)}")
        kind, knots, zl = self.kind.numpy(), self.knots.numpy(), self.levels.numpy()
        center, scale = self.center.numpy(), self.scale.numpy()
        out = v.copy()
        std = kind == L.OSD_XF_STANDARD
        with np.errstate(invalid="ignore", over="ignore"):
            out[std] = (v[std] - center[std]) / scale[std]
        Q = zl.shape[0]
        half = np.float32(0.5)
        for f in np.flatnonzero(kind == L.OSD_XF_QUANTILE_NORMAL):
            x, k = v[f], knots[f]
            if np.isnan(x):
                continue
            lb, ub = int(np.searchsorted(k, x, side="left")), int(np.searchsorted(k, x, side="right"))
            if ub == 0:
                out[f] = zl[0]
            elif lb == Q:
                out[f] = zl[Q - 1]
            elif ub > lb:
                out[f] = half * (zl[(lb + ub - 1) >> 1] + zl[(lb + ub) >> 1])
            else:
                j = lb - 1
                t = (x - k[j]) / (k[j + 1] - k[j])
                out[f] = min(max(zl[j] + t * (zl[j + 1] - zl[j]), zl[j]), zl[j + 1])
        return out

    def map_bounds(self, lo, hi) -> Tuple[np.ndarray, np.ndarray]:
        """Per-feature bounds in data units -> model units (float32 [D] each): the forward map on the finite entries -- it is
        monotone, so lo <= hi is kept -- while an infinite side stays infinite (free)."""
        out = []
        for side in (lo, hi):
            side = np.asarray(side, dtype=np.float32)
            if side.shape != (self.dim,):
                raise ValueError(f"bounds: expected [{self.dim}] values, got {tuple(side.shape)}")
            if np.isnan(side).any():
                raise ValueError("bounds hold NaN: an infinity leaves a side free")
            fin = np.isfinite(side)
            out.append(np.where(fin, self.forward_host(np.where(fin, side, np.float32(0.0))), side).astype(np.float32))
        return out[0], out[1]

    # -- transport ------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Tensors, ints and strings only: loads under ``torch.load(weights_only=True)``."""
        return {"kind": self.kind.clone(), "knots": self.knots.clone(), "levels": self.levels.clone(), "center": self.center.clone(),
                "scale": self.scale.clone(), "blocks": dict(self.blocks), "spec": dict(self.spec), "n_quantiles": self.n_quantiles}

    @classmethod
    def from_state_dict(cls, d: dict) -> "FeatureTransform":
        missing = [k for k in ("kind", "knots", "levels", "center", "scale", "blocks", "spec") if k not in d]
        if missing:
            raise ValueError(f"feature transform state lacks {missing}")
        return cls(d["kind"], d["knots"], d["levels"], d["center"], d["scale"], d["blocks"], d["spec"],
                   d.get("n_quantiles", int(d["levels"].shape[0])))
