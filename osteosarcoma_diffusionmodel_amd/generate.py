"""Generation pipeline on MI355X -- host-side mirror of the reference's utils/generate.py.

``SyntheticPatientGenerator`` keeps the reference's constructor and methods
(utils/generate.py:19-235); ``generate`` runs the whole T-step reverse chain and the
mutation binarisation on the device through ``BiologyAwareDiffusionModel.sample``.
``generate_patients`` is the north-star convenience wrapper.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import pandas as pd
import torch

logger = logging.getLogger(__name__)


def assemble_known(known, n: int, mutation_dim: int, expression_dim: int, pathway_dim: int) -> np.ndarray:
    """float32 [n, D] observation array of ``model.sample(known=...)``: a finite value is observed, NaN is left to the sampler.

    ``known`` is an [n or 1, D] array / tensor, or a dict with any of ``mutations`` / ``expression`` / ``pathways``, each
    [n or 1, its width] (a missing key: the whole block is free).  One row broadcasts to all n.  ValueError on a wrong width, a
    row count other than 1 or n, and on Inf."""
    n = int(n)
    widths = {"mutations": int(mutation_dim), "expression": int(expression_dim), "pathways": int(pathway_dim)}
    D = sum(widths.values())

    def block(v, width, name):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.asarray(v, dtype=np.float32)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim != 2 or v.shape[1] != width:
            raise ValueError(f"known {name}: expected [{n} or 1, {width}], got {tuple(v.shape)}")
        if v.shape[0] not in (1, n):
            raise ValueError(f"known {name}: {v.shape[0]} rows, expected 1 or {n}")
        if np.isinf(v).any():
            raise ValueError(f"known {name} holds Inf: an observation is finite, NaN marks a free element")
        return np.broadcast_to(v, (n, width))

    if isinstance(known, dict):
        extra = set(known) - set(widths)
        if extra:
            raise ValueError(f"known: unknown block(s) {sorted(extra)}; expected any of {list(widths)}")
        out = np.full((n, D), np.nan, dtype=np.float32)
        c0 = 0
        for name, width in widths.items():
            if known.get(name) is not None:
                out[:, c0:c0 + width] = block(known[name], width, name)
            c0 += width
        return out
    return np.array(block(known, D, "features"), dtype=np.float32)        # a copy: the caller's array stays the caller's


def assemble_bounds(spec, mutation_dim: int, expression_dim: int, pathway_dim: int):
    """(lo, hi), two float32 [D] arrays, of ``model.sample(x0_bounds=...)``: the bounds the predicted x0 is clipped to.

    ``spec`` is a ``(lo, hi)`` pair of scalars or [D] arrays, or a dict with any of ``mutations`` / ``expression`` / ``pathways``, each a
    ``(lo, hi)`` pair of scalars or block-wide arrays, or ``None``.  A missing block is free and a ``None`` side is infinite.
    ValueError on a wrong width, a NaN, lo > hi, or an unknown key."""
    widths = {"mutations": int(mutation_dim), "expression": int(expression_dim), "pathways": int(pathway_dim)}
    D = sum(widths.values())

    def side(v, width, fill, name):
        if v is None:
            return np.full(width, fill, dtype=np.float32)
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.asarray(v, dtype=np.float32)
        if v.ndim == 0:
            v = np.full(width, v, dtype=np.float32)
        if v.ndim != 1 or v.shape[0] != width:
            raise ValueError(f"x0_bounds {name}: expected a scalar or [{width}] values, got shape {tuple(v.shape)}")
        if np.isnan(v).any():
            raise ValueError(f"x0_bounds {name} holds NaN: None (or an infinity) leaves a side free")
        return v

    def pair(v, width, name):
        if isinstance(v, (str, bytes, dict)) or not hasattr(v, "__len__") or len(v) != 2:
            raise ValueError(f"x0_bounds {name}: expected a (lo, hi) pair")
        lo, hi = side(v[0], width, -np.inf, name + " lo"), side(v[1], width, np.inf, name + " hi")
        if (lo > hi).any():
            raise ValueError(f"x0_bounds {name}: lo > hi at index {int(np.argmax(lo > hi))}")
        return lo, hi

    if isinstance(spec, dict):
        extra = set(spec) - set(widths)
        if extra:
            raise ValueError(f"x0_bounds: unknown block(s) {sorted(extra)}; expected any of {list(widths)}")
        lo, hi = np.full(D, -np.inf, dtype=np.float32), np.full(D, np.inf, dtype=np.float32)
        c0 = 0
        for name, width in widths.items():
            if spec.get(name) is not None:
                lo[c0:c0 + width], hi[c0:c0 + width] = pair(spec[name], width, name)
            c0 += width
        return lo, hi
    lo, hi = pair(spec, D, "features")
    return np.ascontiguousarray(lo, dtype=np.float32).copy(), np.ascontiguousarray(hi, dtype=np.float32).copy()


class SyntheticPatientGenerator:
    """Generate synthetic patients using a trained model (utils/generate.py:19)."""

    def __init__(self, model, config: dict, device: str = "cuda"):
        self.model = model.to(device)
        self.model.eval()
        # the reference generates 1000 patients per scenario by default (config.yaml:119): small batches, where input_proj's long
        # K loop over few output tiles is the step's longest launch -- let the per-layer engine split it over workgroups unless
        # the caller chose (model.input_splitk = 0 keeps results bit-independent of the batch split)
        if getattr(self.model, "input_splitk", 0) is None:
            self.model.input_splitk = -1
        self.config = config
        self.device = device
        self.mutation_dim = model.mutation_dim
        self.expression_dim = model.expression_dim
        self.pathway_dim = model.pathway_dim
        self.condition_dim = model.condition_dim

    def create_conditions(self, num_samples: int, scenario: Optional[Dict] = None) -> torch.Tensor:
        """Constant condition rows for a scenario, or randn rows (utils/generate.py:39-94)."""
        if scenario is None:
            return torch.randn(num_samples, self.condition_dim, device=self.device)
        values: List[float] = []
        for name in self.config["model"]["condition_on"]:
            if name == "survival_time":
                values.append((scenario.get("survival_time", 800) - 800) / 500)   # hard-wired (800, 500)
            elif name == "event_occurred":
                values.append(scenario.get("event_occurred", 0))
            elif name == "age":
                values.append(scenario.get("age", 15.0))
            elif name == "metastasis_at_diagnosis":
                values.append(scenario.get("metastasis_at_diagnosis", 0))
            # unknown names are skipped, as in the reference
        if len(values) != self.condition_dim:
            logger.warning(f"Condition mismatch: expected {self.condition_dim}, got {len(values)}")
            if len(values) < self.condition_dim:
                values.extend([0.0] * (self.condition_dim - len(values)))
            else:
                values = values[:self.condition_dim]
        row = torch.tensor([values], dtype=torch.float32, device=self.device)
        return row.repeat(num_samples, 1)

    def _guidance_scale(self, guidance_scale: float) -> float:
        """The scale handed to model.sample: the caller's when the model has a null condition, else 1 (today's behaviour)."""
        if float(guidance_scale) != 1.0 and getattr(self.model, "null_condition", None) is None:
            logger.info(f"guidance_scale={guidance_scale} ignored: the model has no null condition "
                        "(config['model']['null_condition']; train with training.condition_dropout > 0)")
            return 1.0
        return float(guidance_scale)

    def _x0_bounds(self, x0_bounds):
        """``x0_bounds`` of generate / generate_scenarios / impute as model.sample takes it: the caller's, else the config's
        ``generation.x0_bounds`` (e.g. ``{mutations: [0, 1], expression: [-4, 4]}``); an absent key changes nothing."""
        if hasattr(self.model, "vae"):
            if x0_bounds is not None and x0_bounds is not False:
                raise ValueError("x0_bounds clips inside the diffusion model's reverse chain and is not accepted for a cVAE model")
            return None                 # the config's default speaks to the diffusion sampler
        if x0_bounds is None:
            x0_bounds = (self.config.get("generation") or {}).get("x0_bounds")
        ft = self._transform()
        if ft is not None and x0_bounds is not None and x0_bounds is not False:
            # the caller speaks data units; the sampler clips in model units (the map is monotone)
            x0_bounds = ft.map_bounds(*assemble_bounds(x0_bounds, self.mutation_dim, self.expression_dim, self.pathway_dim))
        return x0_bounds

    def _solver(self, solver, timestep_spacing) -> dict:
        """``solver`` / ``timestep_spacing`` of generate / generate_scenarios / impute as model.sample's keywords: the caller's, else the
        config's ``generation.solver`` / ``generation.timestep_spacing``; absent keys change nothing."""
        if hasattr(self.model, "vae"):
            if solver is not None or timestep_spacing is not None:
                raise ValueError("solver / timestep_spacing select the diffusion model's sampler and are not accepted for a cVAE model")
            return {}
        gen = self.config.get("generation") or {}
        return {"solver": gen.get("solver") if solver is None else solver,
                "timestep_spacing": gen.get("timestep_spacing", "uniform") if timestep_spacing is None else timestep_spacing}

    def _transform(self):
        """The model's feature transform (``model.feature_transform``) or None.  With one, this class speaks
        data units: ``known`` / ``features`` / ``x0_bounds`` are mapped forward, the samples are mapped back on the device."""
        return getattr(self.model, "feature_transform", None)

    def _known(self, known, n: int):
        """``known`` of generate / generate_scenarios as ``(model, data)``: the device tensor model.sample takes (model units) and the
        caller's values (data units) -- one tensor twice without a feature transform --, or ``(None, None)``.  NaN stays NaN."""
        if known is None:
            return None, None
        data = torch.from_numpy(assemble_known(known, n, self.mutation_dim, self.expression_dim, self.pathway_dim)).to(self.device)
        ft = self._transform()
        return (data if ft is None else ft.forward(data)), data

    def _to_data_units(self, samples: torch.Tensor, known_data=None) -> torch.Tensor:
        """The sampler's output in data units: the inverse map on the device, then the observed elements restored from the caller's
        own values (the inverse of the forward map of a value between two knots can differ from it in the last bits).  Without a
        feature transform: ``samples`` itself."""
        ft = self._transform()
        if ft is None:
            return samples
        samples = ft.inverse(samples, out=samples if samples.dtype == torch.float32 and samples.is_contiguous() else None)
        if known_data is not None:
            samples = torch.where(torch.isnan(known_data), samples, known_data)
        return samples

    @torch.no_grad()
    def generate(self, num_samples: int, scenario: Optional[Dict] = None, guidance_scale: float = 1.0,
                 *, seed: Optional[int] = None, row_offset: int = 0, x_T=None, noise=None, sampling_steps: Optional[int] = None,
                 eta: float = 0.0, known=None, x0_bounds=None, solver: Optional[str] = None,
                 timestep_spacing: Optional[str] = None) -> Dict[str, np.ndarray]:
        """utils/generate.py:96-144.  ``guidance_scale`` is the classifier-free-guidance strength (``model.sample(guidance_scale=w)``:
        1 the plain conditional sampler, larger values follow the scenario more strongly) when the model has a null condition
        (``model.null_condition``: trained with ``training.condition_dropout``).  A model without one -- every reference
        checkpoint -- ignores the value, as the reference does.  The config's ``generation.guidance_scale`` is not read implicitly,
        for the reason ``sampling_steps`` is not.
        Keyword-only extras inject the random draws / shard the Philox stream.  ``sampling_steps=S`` runs the strided DDIM
        sampler (``model.sample(num_inference_steps=S, eta=eta)``); the config's ``generation.sampling_steps`` is not read
        implicitly: ``generate(n, sc, sampling_steps=config["generation"]["sampling_steps"])`` honours it.
        ``known`` (``assemble_known``: an [n or 1, D] array, or a dict of ``mutations`` / ``expression`` / ``pathways`` blocks, NaN =
        free) holds part of every patient fixed: the returned blocks carry the observed values exactly and the rest is sampled
        around them (``model.sample(known=...)``).
        ``x0_bounds`` (``assemble_bounds``: a ``(lo, hi)`` pair or a dict over ``mutations`` / ``expression`` / ``pathways``) clips the
        predicted clean patient of every step to per-feature bounds (``model.sample(x0_bounds=...)``) -- the usual companion of a large
        ``guidance_scale`` and of few ``sampling_steps``; every returned value lies inside its bounds.  Default: the config's
        ``generation.x0_bounds`` when it has one, else ``model.x0_bounds``; ``False`` switches it off.
        ``solver`` (``"ddim"`` or ``"dpmpp_2m"``, the second-order multistep solver: about the accuracy of twice the DDIM steps; needs
        ``sampling_steps`` and ``eta == 0``) and ``timestep_spacing`` (``"uniform"`` or ``"logsnr"``) as in ``model.sample``.  Defaults:
        the config's ``generation.solver`` / ``generation.timestep_spacing`` when it has them, else DDIM on uniform steps.
        A model that carries a feature transform (``model.feature_transform``, from ``data.transform``) is spoken to in DATA units:
        ``known`` and ``x0_bounds`` are mapped forward, the samples are mapped back on the device before the download (a quantile
        column's values lie inside its observed range) and the observed elements are restored from the caller's values.  ``x_T`` /
        ``noise`` are the chain's own draws and ``model.x0_bounds`` is the model's own attribute: model units."""
        x0_bounds = self._x0_bounds(x0_bounds)
        solver_kw = self._solver(solver, timestep_spacing)
        logger.info(f"Generating {num_samples} synthetic patients...")
        if scenario:
            logger.info(f"Scenario: {scenario}")
        conditions = self.create_conditions(num_samples, scenario)
        md, ed = self.mutation_dim, self.expression_dim
        if hasattr(self.model, "vae"):
            # BiologyConstrainedVAE (utils/train.py:233's dispatch; load_trained_model's "cvae" branch): the reference's
            # generate() only ever calls model.sample(conditions, num_samples) and binarises on the host (:124-135)
            if seed is not None or row_offset or x_T is not None or noise is not None:
                raise ValueError("seed / row_offset / x_T / noise drive the diffusion sampler's Philox stream and are not "
                                 "accepted for a cVAE model (pass z= to model.sample directly)")
            if sampling_steps is not None or eta:
                raise ValueError("sampling_steps / eta select the diffusion model's DDIM sampler and are not accepted for a cVAE model")
            if float(guidance_scale) != 1.0:
                raise ValueError("guidance_scale != 1 selects the diffusion model's guided sampler and is not accepted for a cVAE model")
            if known is not None:
                raise ValueError("known conditions the diffusion model's reverse chain and is not accepted for a cVAE model")
            samples = self.model.sample(conditions, num_samples=num_samples).cpu().numpy()
            mutations = (samples[:, :md] > 0.5).astype(float)
        else:
            kn, kn_data = self._known(known, num_samples)
            samples, mask = self.model.sample(conditions, num_samples=num_samples, seed=seed, row_offset=row_offset,
                                              x_T=x_T, noise=noise, return_mutation_mask=True, num_inference_steps=sampling_steps,
                                              eta=eta, guidance_scale=self._guidance_scale(guidance_scale),
                                              known=kn, x0_bounds=x0_bounds, **solver_kw)
            samples = self._to_data_units(samples, kn_data).cpu().numpy()
            # (mutations > 0.5).astype(float), evaluated by the last reverse step's epilogue on the device
            mutations = mask.cpu().numpy().astype(float)
        expression = samples[:, md:md + ed]
        pathways = samples[:, md + ed:]
        logger.info("Generation complete!")
        return {"mutations": mutations, "expression": expression, "pathways": pathways,
                "conditions": conditions.cpu().numpy()}

    def generate_scenarios(self, scenarios: List[Dict], samples_per_scenario: int, *, seed: Optional[int] = None,
                           batched: bool = True, sampling_steps: Optional[int] = None,
                           eta: float = 0.0, guidance_scale: float = 1.0, known=None,
                           x0_bounds=None, solver: Optional[str] = None,
                           timestep_spacing: Optional[str] = None) -> Dict[str, Dict[str, np.ndarray]]:
        """utils/generate.py:146-175: one result dict per scenario name.

        The reference runs the scenarios one after the other, each a chain of T sequential steps.  Rows never interact and the
        conditions are per row, so here all scenarios form ONE batch (scenario k = rows k*N .. (k+1)*N-1) and the chain runs
        once: at the reference's default size (3 scenarios x 1000 patients, config.yaml:119-141) a reverse step is bound by
        launch latency, not by rows, and T steps over 3000 rows cost about what T steps over 1000 do.  ``batched=False`` restores
        the reference's loop (one chain, and one freshly drawn Philox seed, per scenario).  ``sampling_steps`` / ``eta`` select the
        strided DDIM sampler, ``guidance_scale`` the guided one, as in ``generate``.  ``known`` ([samples_per_scenario or 1, D] or a
        dict of blocks, as in ``generate``) holds the same observed values in every scenario: the counterfactual question.
        ``x0_bounds``, ``solver`` and ``timestep_spacing`` as in ``generate``."""
        x0_bounds = self._x0_bounds(x0_bounds)
        solver_kw = self._solver(solver, timestep_spacing)
        if not batched or hasattr(self.model, "vae") or len(scenarios) < 2:
            out = {}
            for scenario in scenarios:
                name = scenario["name"]
                logger.info(f"\nGenerating scenario: {name}")
                out[name] = self.generate(num_samples=samples_per_scenario, scenario=scenario["conditions"],
                                          sampling_steps=sampling_steps, eta=eta, guidance_scale=guidance_scale, known=known,
                                          x0_bounds=x0_bounds, solver=solver, timestep_spacing=timestep_spacing)
            return out
        n = int(samples_per_scenario)
        for scenario in scenarios:
            logger.info(f"\nGenerating scenario: {scenario['name']}")
            logger.info(f"Scenario: {scenario['conditions']}")
        logger.info(f"Generating {len(scenarios)} x {n} synthetic patients in one batch...")
        conditions = torch.cat([self.create_conditions(n, sc["conditions"]) for sc in scenarios], dim=0)
        kn, kn_data = self._known(known, n)
        if kn is not None:
            kn, kn_data = kn.repeat(len(scenarios), 1), kn_data.repeat(len(scenarios), 1)
        with torch.no_grad():
            samples, mask = self.model.sample(conditions, num_samples=conditions.shape[0], seed=seed, return_mutation_mask=True,
                                              num_inference_steps=sampling_steps, eta=eta,
                                              guidance_scale=self._guidance_scale(guidance_scale), known=kn, x0_bounds=x0_bounds,
                                              **solver_kw)
        samples = self._to_data_units(samples, kn_data)
        samples, mask, cond_np = samples.cpu().numpy(), mask.cpu().numpy().astype(float), conditions.cpu().numpy()
        md, ed = self.mutation_dim, self.expression_dim
        out = {}
        for k, scenario in enumerate(scenarios):
            rows = slice(k * n, (k + 1) * n)
            out[scenario["name"]] = {"mutations": mask[rows], "expression": samples[rows, md:md + ed], "pathways": samples[rows, md + ed:],
                                     "conditions": cond_np[rows]}
        logger.info("Generation complete!")
        return out

    def impute(self, features, conditions, *, seed: Optional[int] = None, sampling_steps: Optional[int] = None, eta: float = 0.0,
               guidance_scale: float = 1.0, x0_bounds=None, solver: Optional[str] = None,
               timestep_spacing: Optional[str] = None) -> Dict[str, np.ndarray]:
        """Fill the holes of real rows: ``features`` [n, D] with NaN where a value is missing, ``conditions`` [n, condition_dim] the
        rows' own.  Observed values come back exactly, the holes are sampled around them; returns ``generate``'s dictionary.
        ``x0_bounds`` as in ``generate``: the holes stay inside the bounds, the observed values are the observed values.  ``solver`` and
        ``timestep_spacing`` as in ``generate``."""
        if hasattr(self.model, "vae"):
            raise ValueError("impute conditions the diffusion model's reverse chain and is not accepted for a cVAE model")
        x0_bounds = self._x0_bounds(x0_bounds)
        solver_kw = self._solver(solver, timestep_spacing)
        if isinstance(conditions, torch.Tensor):
            cond = conditions.detach().to(device=self.device, dtype=torch.float32)
        else:
            cond = torch.as_tensor(np.asarray(conditions, dtype=np.float32), device=self.device)
        if cond.dim() != 2 or cond.shape[1] != self.condition_dim:
            raise ValueError(f"conditions: expected [n, {self.condition_dim}], got {tuple(cond.shape)}")
        n = cond.shape[0]
        rows = features.shape[0] if hasattr(features, "shape") and len(features.shape) == 2 else None
        if rows != n:
            raise ValueError(f"features: expected [{n}, D] (one row per condition row)")
        md, ed = self.mutation_dim, self.expression_dim
        with torch.no_grad():
            kn, kn_data = self._known(features, n)
            samples, mask = self.model.sample(cond, num_samples=n, seed=seed, return_mutation_mask=True, num_inference_steps=sampling_steps,
                                              eta=eta, guidance_scale=self._guidance_scale(guidance_scale), known=kn,
                                              x0_bounds=x0_bounds, **solver_kw)
            samples = self._to_data_units(samples, kn_data)
        samples = samples.cpu().numpy()
        return {"mutations": mask.cpu().numpy().astype(float), "expression": samples[:, md:md + ed], "pathways": samples[:, md + ed:],
                "conditions": cond.cpu().numpy()}

    def counterfactual(self, features, conditions, scenario: Optional[Dict] = None, *, new_conditions=None, keep=None,
                       method: str = "ddpm", sampling_steps: int = 50, strength: float = 0.6, eta: float = 1.0,
                       guidance_scale: float = 1.0, x0_bounds=None, seed: Optional[int] = None) -> Dict[str, np.ndarray]:
        """What would these patients look like under another condition?  ``features`` are real rows in data units -- an [n, D] array or
        a dict with all of ``mutations`` / ``expression`` / ``pathways`` --, ``conditions`` [n, condition_dim] the rows' own.  Each row
        is inverted under its own condition and decoded under the new one (``model.edit``), so a row and its
        counterfactual are a pair: the same patient-specific noise, another condition.

        Exactly one of ``scenario`` (a dict as in ``generate``: the named conditions are overridden in every row, the others keep the
        row's own values) and ``new_conditions`` ([n, condition_dim], full rows) says what changes.  ``keep`` holds columns at their
        observed values through the decode (``sample``'s ``known``): a dict over the blocks with ``True`` (the whole block) or a boolean
        mask of the block's width, or a boolean [D] mask -- ``keep={"mutations": True}`` asks for the same tumour genotype under another
        outcome.  ``method`` / ``sampling_steps`` / ``strength`` / ``eta`` as in ``model.invert``: ``strength`` is how far up the rows are
        noised, so how much may change.  ``guidance_scale`` and ``x0_bounds`` apply to the decode, as in ``generate``.

        A model with a feature transform is spoken to in data units, as by ``impute``: forward in front, inverse behind, kept values
        restored from the caller's.  Returns ``generate``'s dictionary (``conditions``: the new rows) plus ``original_conditions``."""
        if hasattr(self.model, "vae"):
            raise ValueError("counterfactual inverts the diffusion model's reverse chain and is not accepted for a cVAE model")
        if (scenario is None) == (new_conditions is None):
            raise ValueError("counterfactual: give exactly one of scenario and new_conditions")

        def cond_rows(c, name):
            if isinstance(c, torch.Tensor):
                c = c.detach().to(device=self.device, dtype=torch.float32)
            else:
                c = torch.as_tensor(np.asarray(c, dtype=np.float32), device=self.device)
            if c.dim() != 2 or c.shape[1] != self.condition_dim:
                raise ValueError(f"{name}: expected [n, {self.condition_dim}], got {tuple(c.shape)}")
            return c.contiguous()

        cond = cond_rows(conditions, "conditions")
        n = cond.shape[0]
        if new_conditions is not None:
            new = cond_rows(new_conditions, "new_conditions")
            if new.shape[0] != n:
                raise ValueError(f"new_conditions: {new.shape[0]} rows, conditions has {n}")
        else:
            names = list(self.config["model"]["condition_on"])[:self.condition_dim]
            unknown = set(scenario) - set(names)
            if unknown:
                raise ValueError(f"scenario names {sorted(unknown)}, the model is conditioned on {names}")
            encoded = self.create_conditions(1, scenario)[0]
            new = cond.clone()
            for j, name in enumerate(names):
                if name in scenario:
                    new[:, j] = encoded[j]
        md, ed, pd_ = self.mutation_dim, self.expression_dim, self.pathway_dim
        D = md + ed + pd_
        data_np = assemble_known(features, n, md, ed, pd_)
        if np.isnan(data_np).any():
            raise ValueError("features: a counterfactual needs complete rows (impute fills holes)")
        data = torch.from_numpy(data_np).to(self.device)
        keep_mask = np.zeros(D, dtype=bool)
        if isinstance(keep, dict):
            widths = {"mutations": md, "expression": ed, "pathways": pd_}
            extra = set(keep) - set(widths)
            if extra:
                raise ValueError(f"keep: unknown block(s) {sorted(extra)}; expected any of {list(widths)}")
            c0 = 0
            for name, width in widths.items():
                v = keep.get(name)
                if v is not None and v is not False:
                    m = np.ones(width, dtype=bool) if v is True else np.asarray(v, dtype=bool).reshape(-1)
                    if m.shape[0] != width:
                        raise ValueError(f"keep {name}: expected True or a boolean mask of {width} columns")
                    keep_mask[c0:c0 + width] = m
                c0 += width
        elif keep is not None:
            keep_mask = np.asarray(keep, dtype=bool).reshape(-1)
            if keep_mask.shape[0] != D:
                raise ValueError(f"keep: expected a dict over the blocks or a boolean mask of {D} columns")
        x0_bounds = self._x0_bounds(x0_bounds)
        ft = self._transform()
        with torch.no_grad():
            x_model = data if ft is None else ft.forward(data)
            kn = kn_data = None
            if keep_mask.any():
                km = torch.from_numpy(keep_mask).to(self.device)
                nan = torch.full_like(data, float("nan"))
                kn_data = torch.where(km[None, :], data, nan)
                kn = torch.where(km[None, :], x_model, nan)
            rec = self.model.invert(x_model, cond, method=method, num_inference_steps=sampling_steps, strength=strength, eta=eta, seed=seed)
            zs = rec.noise if rec.noise is not None and rec.noise.shape[0] > 0 else None
            samples, mask = self.model.sample(new, num_samples=n, x_T=rec.x_start, noise=zs, seed=0, return_mutation_mask=True, eta=rec.eta,
                                              guidance_scale=self._guidance_scale(guidance_scale), known=kn, x0_bounds=x0_bounds,
                                              timesteps=rec.timesteps)
            samples = self._to_data_units(samples, kn_data)
        samples = samples.cpu().numpy()
        return {"mutations": mask.cpu().numpy().astype(float), "expression": samples[:, md:md + ed], "pathways": samples[:, md + ed:],
                "conditions": new.cpu().numpy(), "original_conditions": cond.cpu().numpy()}

    def save_synthetic_data(self, synthetic_data: Dict[str, np.ndarray], output_dir: Path,
                            gene_names: Dict[str, List[str]], prefix: str = "synthetic"):
        """Four CSVs per scenario (utils/generate.py:177-235)."""
        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        for key, cols_key, stem in (("mutations", "mutation_genes", "mutations"),
                                    ("expression", "expression_genes", "expression"),
                                    ("pathways", "pathway_names", "pathways")):
            if cols_key in gene_names:
                path = output_dir / f"{prefix}_{stem}.csv"
                pd.DataFrame(synthetic_data[key], columns=gene_names[cols_key]).to_csv(path, index=False)
                logger.info(f"Saved {stem} to {path}")
        cond_path = output_dir / f"{prefix}_conditions.csv"
        pd.DataFrame(synthetic_data["conditions"], columns=self.config["model"]["condition_on"]).to_csv(cond_path, index=False)
        logger.info(f"Saved conditions to {cond_path}")


def checkpoint_prediction_type(checkpoint: dict, config: dict) -> Optional[str]:
    """The prediction type a model built from ``config`` must take over from ``checkpoint``: the checkpoint's when ``config`` names
    none, None when there is nothing to take over.  Both naming different types is a ValueError -- sampling a v-trained network as an
    epsilon one returns noise without any other sign.  A checkpoint without the key (every reference checkpoint) is an epsilon model."""
    from .objective import check_prediction_type
    saved = ((checkpoint.get("config") or {}).get("model") or {}).get("diffusion", {}).get("prediction_type")
    asked = ((config or {}).get("model") or {}).get("diffusion", {}).get("prediction_type")
    saved_type = check_prediction_type("epsilon" if saved is None else saved)
    if asked is None:
        return None if saved is None else saved_type
    if check_prediction_type(asked) != saved_type:
        raise ValueError(f"config['model']['diffusion']['prediction_type'] is {asked!r} but the checkpoint was trained with {saved_type!r}")
    return None


def checkpoint_mutation_link(checkpoint: dict, config: dict) -> Optional[str]:
    """``checkpoint_prediction_type`` for ``mutation_link``: the checkpoint's link when ``config`` names none, None when there is
    nothing to take over, ValueError when both name different links -- a logit read as x0^ gives no other sign.  A checkpoint without
    the key is an identity model."""
    from .objective import check_mutation_link
    saved = ((checkpoint.get("config") or {}).get("model") or {}).get("diffusion", {}).get("mutation_link")
    asked = ((config or {}).get("model") or {}).get("diffusion", {}).get("mutation_link")
    saved_link = check_mutation_link("identity" if saved is None else saved)
    if asked is None:
        return None if saved is None else saved_link
    if check_mutation_link(asked) != saved_link:
        raise ValueError(f"config['model']['diffusion']['mutation_link'] is {asked!r} but the checkpoint was trained with {saved_link!r}")
    return None


def load_trained_model(checkpoint_path: Path, config: dict, device: str, use_ema: Optional[bool] = None):
    """Checkpoint -> model (utils/generate.py:238-298): condition width from the saved
    ``condition_embed.mlp.0.weight``, feature dims from the processed CSV headers.
    ``use_ema``: which weights of a checkpoint written with ``training.ema_decay`` -- None (default) the averaged ones
    (``ema_state_dict``) when the file has them, else ``model_state_dict``; False always ``model_state_dict`` (the last iterate);
    True the averaged ones, KeyError when the file has none.
    ``prediction_type`` (what the network was trained to predict) travels in the checkpoint's own config: a ``config`` without the key
    adopts the checkpoint's, one that names a different type than the checkpoint raises ValueError; ``mutation_link`` likewise, and
    ``data.transform`` (the checkpoint's ``feature_transform`` tables become ``model.feature_transform``; a config naming another spec
    raises ValueError)."""
    from .diffusion import BiologyAwareDiffusionModel
    logger.info(f"Loading model from {checkpoint_path}")
    checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    has_ema = "ema_state_dict" in checkpoint
    if use_ema and not has_ema:
        raise KeyError(f"use_ema=True but {checkpoint_path} has no ema_state_dict (train with training.ema_decay)")
    if has_ema and (use_ema is None or use_ema):
        from .train import ParamEMA
        state_dict = ParamEMA.model_state(checkpoint["ema_state_dict"])
        logger.info(f"Loaded the EMA weights (ema_state_dict, {int(checkpoint['ema_state_dict'].get('num_updates', 0))} updates)")
    else:
        state_dict = checkpoint["model_state_dict"]
        logger.info("Loaded the last iterate (model_state_dict)" + ("; the checkpoint also has EMA weights" if has_ema else ""))
    arch = config["model"]["architecture"]
    if arch not in ("diffusion", "cvae"):
        raise ValueError(f"Unknown architecture: {arch}")
    saved_pred = checkpoint_prediction_type(checkpoint, config) if arch == "diffusion" else None
    saved_link = checkpoint_mutation_link(checkpoint, config) if arch == "diffusion" else None
    # data.transform travels as the checkpoint's own tables; a config that names another spec is refused (the prediction_type rule)
    from .transform import checkpoint_feature_transform, transform_config
    if arch == "cvae" and (transform_config(config) is not None or "feature_transform" in checkpoint):
        raise ValueError("data.transform maps the diffusion model's features and is not accepted for a cVAE model")
    saved_transform = checkpoint_feature_transform(checkpoint, config) if arch == "diffusion" else None
    processed = Path(config["data"]["processed_dir"])
    dims = []
    for fname in ("mutation_matrix_aligned.csv", "expression_matrix_aligned.csv", "pathway_scores.csv"):
        dims.append(pd.read_csv(processed / fname, index_col=0, nrows=1).shape[1])
    if arch == "diffusion":
        saved_cond_dim = state_dict["condition_embed.mlp.0.weight"].shape[1]
        build_config = config
        if saved_pred is not None or saved_link is not None:
            # what the checkpoint hands over is in place when the constructor checks that link and type go together; the caller's
            # config is left alone
            import copy
            build_config = copy.deepcopy(config)
            dm = build_config["model"]["diffusion"]
            if saved_pred is not None:
                dm["prediction_type"] = saved_pred
            if saved_link is not None:
                dm["mutation_link"] = saved_link
        model = BiologyAwareDiffusionModel(mutation_dim=dims[0], expression_dim=dims[1], pathway_dim=dims[2],
                                           condition_dim=saved_cond_dim, config=build_config)
    else:
        # the reference reads the diffusion key even for a cVAE checkpoint (utils/generate.py:250) and fails on it;
        # here the condition width comes from the encoder's first Linear: in_features = data_dim + condition_dim
        from .cvae import BiologyConstrainedVAE
        saved_cond_dim = state_dict["vae.encoder.mlp.0.weight"].shape[1] - sum(dims)
        model = BiologyConstrainedVAE(mutation_dim=dims[0], expression_dim=dims[1], pathway_dim=dims[2],
                                      condition_dim=saved_cond_dim, config=config)
    model.load_state_dict(state_dict)
    # the null condition of classifier-free guidance is no parameter: it travels in the checkpoint's own config
    saved_null = (checkpoint.get("config") or {}).get("model", {}).get("null_condition")
    if arch == "diffusion" and model.null_condition is None and saved_null is not None:
        model.null_condition = [float(v) for v in saved_null]
    if saved_pred is not None:
        model.prediction_type = saved_pred
    if saved_link is not None:
        model.mutation_link = saved_link
    if saved_transform is not None:
        if saved_transform.blocks != {"mutations": dims[0], "expression": dims[1], "pathways": dims[2]}:
            raise ValueError(f"the checkpoint's data.transform was fitted on blocks {saved_transform.blocks}, the processed data has {dims}")
        model.feature_transform = saved_transform
    model.to(device)
    model.eval()
    logger.info("Model loaded successfully!")
    return model


def generate_patients(model_or_checkpoint, config: dict, num_samples: int, scenario: Optional[Dict] = None,
                      device: Optional[str] = None, use_ema: Optional[bool] = None, **kw) -> Dict[str, np.ndarray]:
    """north_star name: load (if given a path; ``use_ema`` as in ``load_trained_model``) and run SyntheticPatientGenerator.generate."""
    device = device or "cuda"
    model = model_or_checkpoint
    if isinstance(model_or_checkpoint, (str, Path)):
        model = load_trained_model(Path(model_or_checkpoint), config, device, use_ema=use_ema)
    return SyntheticPatientGenerator(model, config, device).generate(num_samples, scenario, **kw)
