"""BiologyAwareDiffusionModel on MI355X -- host-side mirror of the reference's
models/diffusion.py:259-449.

Same constructor, attributes, ``state_dict`` keys and methods (``forward``,
``q_sample``, ``p_sample``, ``sample``) as the reference class, so
``utils/train.py``-style trainers and ``utils/generate.py``-style generators
work unchanged; every method runs hand-written HIP kernels through the C ABI
of ``libosdiff.so`` (include/osdiff.h).  There is no CPU path: tensors must
live on a ROCm device.

Build-only additions are keyword-only and default-off (``noise=``, ``x_T=``,
``seed=``, ``t=``, ``dropout_masks=``): they inject the random draws for parity
tests.  Without them randomness comes from the library's Philox stream, seeded
from torch's default generator (so ``torch.manual_seed`` makes runs repeatable).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L

COND_EMBED_WIDTH = 64  # literal of models/diffusion.py:285


class PathwayGraphEncoder(nn.Module):
    """Name kept importable for API parity (models/diffusion.py:14-88).  The reference
    never instantiates it and it is not part of the hot path; it needs torch_geometric."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError("PathwayGraphEncoder is dead code in the reference and is not provided")


class ConditionalEmbedding(nn.Module):
    """Parameter container for Linear -> SiLU -> Linear (models/diffusion.py:91-114)."""

    def __init__(self, num_continuous: int, embedding_dim: int):
        super().__init__()
        self.num_continuous = num_continuous
        self.embedding_dim = embedding_dim
        self.mlp = nn.Sequential(nn.Linear(num_continuous, embedding_dim), nn.SiLU(),
                                 nn.Linear(embedding_dim, embedding_dim))


class TimeEmbedding(nn.Module):
    """Sinusoidal embedding of t in [0,1) (models/diffusion.py:117-139); host-side table builder."""

    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim

    def forward(self, t):
        half = self.dim // 2
        step = np.log(10000) / (half - 1)
        freq = torch.exp(torch.arange(half, device=t.device) * -step)
        arg = t[:, None] * freq[None, :]
        return torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)


def _block(cin: int, cout: int, p: float) -> nn.Sequential:
    # indices 0,1,4,5 carry the parameters, as in models/diffusion.py:200-208
    return nn.Sequential(nn.Linear(cin, cout), nn.GroupNorm(8, cout), nn.SiLU(), nn.Dropout(p),
                         nn.Linear(cout, cout), nn.GroupNorm(8, cout), nn.SiLU())


class DiffusionUNet(nn.Module):
    """Parameter container with the reference's module names (models/diffusion.py:142-196).
    Construction order matches the reference so a given torch seed yields the same init."""

    def __init__(self, data_dim, time_dim=128, condition_dim=64, hidden_dims=(256, 512, 256), dropout=0.1):
        super().__init__()
        hidden_dims = list(hidden_dims)
        self.data_dim = data_dim
        self.time_embed = TimeEmbedding(time_dim)
        self.input_proj = nn.Linear(data_dim, hidden_dims[0])
        self.cond_proj = nn.Linear(condition_dim, hidden_dims[0])
        self.time_proj = nn.Linear(time_dim, hidden_dims[0])
        self.encoder = nn.ModuleList()
        cin = hidden_dims[0]
        for h in hidden_dims[1:]:
            self.encoder.append(_block(cin, h, dropout))
            cin = h
        self.bottleneck = _block(cin, cin, dropout)
        self.decoder = nn.ModuleList()
        cur = hidden_dims[-1]
        for i in range(len(hidden_dims) - 2, -1, -1):
            self.decoder.append(_block(cur + hidden_dims[i + 1], hidden_dims[i], dropout))
            cur = hidden_dims[i]
        self.output_proj = nn.Linear(cur, data_dim)


def _draw_seed() -> int:
    """63-bit seed from torch's default CPU generator (follows torch.manual_seed)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


class _Engine:
    """Owns the osd_handle for one device and keeps its borrowed pointers current."""

    def __init__(self, model: "BiologyAwareDiffusionModel", device: torch.device):
        lib = L.lib()
        cfg = L.OsdConfig()
        cfg.mutation_dim, cfg.expression_dim = model.mutation_dim, model.expression_dim
        cfg.pathway_dim, cfg.condition_dim = model.pathway_dim, model.condition_dim
        cfg.time_dim = model._time_dim
        hd = model._hidden_dims
        if len(hd) > L.OSD_MAX_HIDDEN:
            raise ValueError(f"at most {L.OSD_MAX_HIDDEN} hidden dims are supported")
        cfg.n_hidden = len(hd)
        for i, v in enumerate(hd):
            cfg.hidden_dims[i] = int(v)
        cfg.num_steps = model.num_steps
        cfg.dropout_p = float(model._dropout_p)
        cfg.device = device.index if device.index is not None else torch.cuda.current_device()
        self.cfg = cfg
        self.device = device
        self.handle = C.c_void_p()
        L.check(lib.osd_create(C.byref(cfg), C.byref(self.handle)))
        self.n_params = lib.osd_num_params(C.byref(cfg))
        # schedule + time-embedding tables, computed on the host with the reference's expressions
        T = model.num_steps
        abar = model.alphas_cumprod.detach().float().cpu()
        betas = model.betas.detach().float().cpu()
        coef = torch.zeros(T, 6, dtype=torch.float32)
        for t in range(T):                       # 0-d tensor arithmetic, order of models/diffusion.py:401-419
            alpha_t = 1.0 - betas[t]
            ab = abar[t]
            coef[t, 0] = torch.sqrt(1 - ab)
            coef[t, 1] = torch.sqrt(ab)
            coef[t, 3] = 1 - ab
            if t > 0:
                abp = abar[t - 1]
                coef[t, 2] = torch.sqrt(abp) * betas[t]
                coef[t, 4] = torch.sqrt(alpha_t) * (1 - abp)
                coef[t, 5] = torch.sqrt((1 - abp) / (1 - ab) * betas[t])
        t_norm = torch.arange(T).float() / T     # == python t / T for every t < T
        temb = TimeEmbedding(model._time_dim)(t_norm).contiguous()
        sa = model.sqrt_alphas_cumprod.detach().float().cpu().contiguous()
        s1 = model.sqrt_one_minus_alphas_cumprod.detach().float().cpu().contiguous()
        L.check(lib.osd_set_schedule(self.handle, L.ptr(sa), L.ptr(s1), L.ptr(coef.contiguous()), L.ptr(temb)))
        self._sig = None
        self.constraints_version = 0
        self.loss_state = None          # the model's _loss_state() this handle was last configured with (None: the library's default)
        self.prediction_type = "epsilon"  # the model's prediction_type this handle's tables were last folded for (the library's default)
        self.serial = 0                 # bumped by every call that rewrites the handle's training workspace
        self.dp_clip = 0.0              # the per-row gradient bound this handle was last given (osd_set_dp_clip; 0: off, the library's default)
        self.loss_mask = False          # whether this handle was last told to mask NaN (osd_set_loss_mask; off: the library's default)
        self.n_link = 0                 # the logistic columns this handle was last given (osd_set_output_link; 0: off, the library's default)

    def set_output_link(self, n_link: int):
        L.check(L.lib().osd_set_output_link(self.handle, int(n_link)))
        self.n_link = int(n_link)

    def set_loss_mask(self, model: "BiologyAwareDiffusionModel"):
        """Validate the model's missing_values and hand it to the handle (osd_set_loss_mask: persistent)."""
        on = check_missing_values(getattr(model, "missing_values", None)) == "mask"
        L.check(L.lib().osd_set_loss_mask(self.handle, int(on)))
        self.loss_mask = on

    def set_dp_clip(self, model: "BiologyAwareDiffusionModel"):
        """Validate the model's dp_max_grad_norm and hand it to the handle (osd_set_dp_clip: persistent)."""
        c = getattr(model, "dp_max_grad_norm", None)
        c = 0.0 if c is None else float(c)
        L.check(L.lib().osd_set_dp_clip(self.handle, c))        # ValueError for a negative or non-finite bound
        self.dp_clip = c

    def set_constraints(self, spec):
        lib = L.lib()
        if spec is None:
            L.check(lib.osd_set_constraints(self.handle, None))
            return
        from .constraints import csr_from_pathways
        off, mem = csr_from_pathways(spec["pathways"])
        ca = np.ascontiguousarray(spec["cols_a"], dtype=np.int32)
        cb = np.ascontiguousarray(spec["cols_b"], dtype=np.int32)
        c = L.OsdConstraints()
        i32p = C.POINTER(C.c_int32)
        c.pathway_offsets, c.pathway_members, c.n_pathways = off.ctypes.data_as(i32p), mem.ctypes.data_as(i32p), len(off) - 1
        c.pathway_weight = spec["w_pc"]
        c.cols_a, c.cols_b, c.n_a, c.n_b = ca.ctypes.data_as(i32p), cb.ctypes.data_as(i32p), len(ca), len(cb)
        c.mutexpr_weight = spec["w_me"]
        L.check(lib.osd_set_constraints(self.handle, C.byref(c)))

    def set_prediction(self, model: "BiologyAwareDiffusionModel"):
        """Validate the model's prediction_type and refold the handle's step tables for it (osd_set_prediction: persistent)."""
        from . import objective as OB
        kind = OB.PREDICTION_TYPES[OB.check_prediction_type(model.prediction_type)]
        L.check(L.lib().osd_set_prediction(self.handle, kind))

    def set_loss(self, model: "BiologyAwareDiffusionModel"):
        """Validate the model's objective attributes and hand them to the handle (osd_set_loss: persistent)."""
        from . import objective as OB
        kind = OB.LOSS_KINDS[OB.check_loss_type(model.loss_type)]
        delta = OB.check_huber_delta(model.huber_delta)
        table = OB.loss_table(OB.check_loss_weighting(model.loss_weighting), OB.check_gamma(model.min_snr_gamma), model.alphas_cumprod,
                              model._loss_weights, OB.check_prediction_type(model.prediction_type))
        L.check(L.lib().osd_set_loss(self.handle, kind, delta, None if table is None else table.ctypes.data))

    def close(self):
        if self.handle:
            L.lib().osd_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self, model: "BiologyAwareDiffusionModel"):
        """Bind the current stream; re-hand the parameter pointers if any tensor moved or changed."""
        lib = L.lib()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(lib.osd_set_stream(self.handle, C.c_void_p(stream)))
        params = model._param_list()
        sig = tuple((p.data_ptr(), p._version) for p in params)
        if sig != self._sig:
            for p in params:
                if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
                    raise RuntimeError("parameters must be contiguous fp32 tensors on the model's device")
            arr = L.ptr_array(params)
            L.check(lib.osd_load_weights(self.handle, arr, len(params)))
            self._sig = sig


def check_missing_values(v):
    """``missing_values``: None (the default: NaN is not accepted in x_0) or "mask" (NaN = not observed, masked out of the loss)."""
    if v is not None and v != "mask":
        raise ValueError(f"missing_values must be None or 'mask', got {v!r}")
    return v


def _if_truthy(v):
    return int(v) if v else None


def _if_set(v):
    return None if v is None else int(v)


def _choice(values: dict, message: str):
    def encode(v):
        try:
            return values[v]
        except (KeyError, TypeError):
            raise ValueError(f"{message}, got {v!r}") from None
    return encode


# The model's library tunables, applied in this order by every engine lookup: (model attribute, osd_set_option name, encoder).
# The encoder turns the attribute into the option's value, or None to leave the library's own value; a value it does not know
# raises ValueError.
ENGINE_OPTIONS = (
    ("sample_chunk_rows", "chunk_rows", _if_truthy),
    ("sample_streams", "n_streams", _if_truthy),
    ("train_streams", "train_streams", _if_truthy),
    ("train_squad", "train_squad", _if_set),
    ("cond_bwd_fused", "cond_bwd_fused", lambda v: None if v is None else int(bool(v))),
    ("sampler", "sampler", _choice({"auto": 0, "chain": 1, "graph": 2, "layers": 2}, "sampler must be 'auto', 'chain' or 'graph'")),
    ("chain_variant", "chain_variant", _choice({None: 0, "auto": 0, "workspace": 1, "panel": 2, "squad": 3},
                                               "chain_variant must be None, 'auto', 'workspace', 'panel' or 'squad'")),
    ("squad_panel", "squad_panel", _choice({None: 0, 0: 0, 16: 16, 32: 32}, "squad_panel must be None, 16 or 32")),
    ("precision", "precision", _choice({None: 0, "fp32": 0, "f32": 0, "bf16x3": 1}, "precision must be None, 'fp32' or 'bf16x3'")),
    ("chain_grid", "chain_grid", _if_set),
    ("chain_steps_per_launch", "chain_steps_per_launch", _if_set),
    ("chain_stagger", "chain_stagger", _if_set),
    ("chain_spin_budget", "chain_spin_budget", _if_set),
    ("chain_wall_budget_ms", "chain_wall_budget_ms", _if_set),
    ("input_splitk", "input_splitk", _if_set),
    ("bound_rows", "bound_rows", _if_set),
)


class BiologyAwareDiffusionModel(nn.Module):
    """Drop-in for models/diffusion.py:259 -- see module docstring."""

    def __init__(self, mutation_dim: int, expression_dim: int, pathway_dim: int, condition_dim: int, config: dict):
        super().__init__()
        self.mutation_dim = mutation_dim
        self.expression_dim = expression_dim
        self.pathway_dim = pathway_dim
        self.condition_dim = condition_dim
        self.data_dim = mutation_dim + expression_dim + pathway_dim

        m = config["model"]
        self._time_dim = int(m["latent_dim"])
        self._hidden_dims = [int(v) for v in m["hidden_dims"]]
        self._dropout_p = float(m["gnn"]["dropout"])          # the GNN key, as models/diffusion.py:294
        for h in self._hidden_dims:
            if h % 8:
                raise ValueError("num_channels must be divisible by num_groups")   # nn.GroupNorm's message
        if self._time_dim // 2 != COND_EMBED_WIDTH:
            raise ValueError("config.model.latent_dim // 2 must equal 64: the reference's ConditionalEmbedding "
                             "is 64 wide while cond_proj expects latent_dim // 2 inputs (models/diffusion.py:285,292)")

        self.condition_embed = ConditionalEmbedding(num_continuous=condition_dim, embedding_dim=COND_EMBED_WIDTH)
        self.unet = DiffusionUNet(data_dim=self.data_dim, time_dim=self._time_dim,
                                  condition_dim=self._time_dim // 2, hidden_dims=self._hidden_dims,
                                  dropout=self._dropout_p)

        self.num_steps = int(m["diffusion"]["num_steps"])
        self.register_buffer("betas", self._get_beta_schedule(m["diffusion"]["beta_schedule"], self.num_steps))
        alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.register_buffer("alphas_cumprod", alphas_cumprod)
        self.register_buffer("sqrt_alphas_cumprod", torch.sqrt(alphas_cumprod))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - alphas_cumprod))
        self._engines = {}
        # sampling tunables forwarded to the library (rows per chunk, chunks in flight, hipGraph replay)
        self.sample_chunk_rows: Optional[int] = None
        self.sample_streams: Optional[int] = None
        self.use_graph: bool = True
        # reverse-chain engine: "auto" (library default: the persistent chain kernel for large eval-mode batches of a
        # 256/512-wide architecture, else the per-layer kernels), "chain", "graph" (per-layer kernels; hipGraph iff use_graph)
        self.sampler: str = "auto"
        # which chain kernel: "workspace" (csrc/chain.h: 128-row tiles, activations through a private workspace -- the faster one from
        # 65 536 rows on), "panel" (csrc/chain_panel.h: 64 patients per workgroup, activations in LDS; bit-identical; at its full
        # rate from 16 384 rows on; architectures whose panels do not fit run the workspace kernel), None / "auto" (the library's choice:
        # workspace from 65 536 rows on, panel from 10 240 rows on, squad up to 3 072 rows), "squad" (csrc/chain_squad.h: eight workgroups per
        # 32 patients, the small-batch kernel; agrees with the other engines to fp32 rounding, not bitwise; batches it cannot keep resident run
        # on auto's other choices)
        self.chain_variant: Optional[str] = None
        self.last_chain_variant: Optional[str] = None     # the one the most recent chain-kernel sample() used
        # patients per panel of the squad chain: None (the library's choice: 16 up to one 32-patient workgroup per CU -- ~1 000 rows --, else 32), 16, 32
        self.squad_panel: Optional[int] = None
        self.last_squad_panel: Optional[int] = None
        self.chain_grid: Optional[int] = None             # workgroup count of the chain kernel (tests)
        self.chain_steps_per_launch: Optional[int] = None
        self.chain_stagger: Optional[int] = None
        self.chain_spin_budget: Optional[int] = None      # ticks (100 MHz) a dependency wait inside the chain kernel may take
        self.chain_wall_budget_ms: Optional[int] = None   # host-side budget of a chain (0 / None: 10 x the estimate + 2 s)
        # per-layer engine, input_proj split-K over workgroups (small-batch latency path): None / 0 off -- a row's result is then
        # independent of chunking and sharding, bit for bit --, -1 auto (chunks with < 128 input_proj tiles), n = slices.
        # SyntheticPatientGenerator switches None to auto: its per-scenario batches are the reference's default workload
        self.input_splitk: Optional[int] = None
        self.last_sampler: Optional[str] = None           # engine the most recent sample() ran on
        # rows per launch group of the likelihood sweep (variational_bound / row_sq_error) and of invert(method="ddpm"): None = the
        # library's 32 768.  It caps the training workspace they run in
        self.bound_rows: Optional[int] = None
        # arithmetic of the eval-mode forward / p_sample / sample GEMMs: None / "fp32" = v_mfma_f32_32x32x2_f32, the reference's F.linear in
        # fp32 (models/diffusion.py:198-256; the default); "bf16x3" = every fp32 operand as three bf16 planes (exact) and six bf16 MFMAs
        # per product with fp32 accumulation (csrc/gemm_bf3.h): fp32 accuracy -- the same stated tolerances -- at the bf16 matrix rate.
        # Trunk widths 256 / 512 only; train-mode (dropout) calls and training stay fp32.
        self.precision: Optional[str] = None
        self.last_precision: Optional[str] = None         # what the most recent predict_noise / p_sample / sample computed in
        self.train_streams: Optional[int] = None      # 1 = whole backward on one stream, 2 (library default) = weight gradients on a side stream
        # the ten Linear+GroupNorm+SiLU layers of a training forward pass as one launch of squads (csrc/train_squad.h) from 2 048 rows on:
        # None / True (library default) or False (per-layer launches)
        self.train_squad = None       # None (library default) | False / 0 | True / 1 (forward only) | 2 (forward and the dgrad chain, csrc/train_squad_bwd.h)
        # the conditioning branch's backward below h0 (time-table scatter, two 64-wide dgrads, SiLU backward) as one launch
        # (k_cond_bwd, csrc/k_train.hip): None / True (library default) or False (four launches)
        self.cond_bwd_fused = None
        # classifier-free guidance: the null condition c0 (condition_dim floats), the condition the model saw in the rows condition dropout
        # replaced (train.py: training.condition_dropout) and the unconditional branch of guided sampling (sample / predict_noise:
        # guidance_scale).  A plain attribute -- no parameter, no buffer: it goes through condition_embed / cond_proj like any condition,
        # and state_dict() keeps the reference's keys.  None: the model has none (every reference checkpoint)
        self.null_condition = m.get("null_condition")
        # per-feature bounds the predicted x0 is clipped to inside every sampling step (sample(x0_bounds=...); generate.assemble_bounds
        # describes the forms: a (lo, hi) pair or a dict over mutations / expression / pathways).  None: no clipping, today's sampler
        self.x0_bounds = None
        # the feature transform the training data went through (transform.FeatureTransform; config['data']['transform'], DESIGN.md section
        # 3.27).  A plain attribute like null_condition: the Trainer adopts the dataset's, checkpoints carry its tables, and the
        # generator maps between data units and model units with it.  Everything on this class -- sample, p_sample, predict*,
        # variational_bound, row_sq_error, loss_profile, x0_bounds, known -- stays in MODEL units.  None: the model sees the data as is
        self.feature_transform = None
        # optional constraint losses (set_constraints); None = the reference's eps-MSE only
        self._constraints = None
        self._constraints_version = 0
        # the eps-loss of the training step (objective.py): config['model']['diffusion'] keys loss_type ("l2" -- the reference's MSE and
        # the default --, "l1", "huber"), huber_delta, loss_weighting (None | "min_snr") and min_snr_gamma.  Plain attributes: assigning
        # one takes effect at the next training call (an unknown value raises ValueError there); checkpoints carry them in the config
        from . import objective as OB
        dm = m["diffusion"]
        self.loss_type: str = OB.check_loss_type(dm.get("loss_type", "l2"))
        self.huber_delta: float = OB.check_huber_delta(dm.get("huber_delta", 1.0))
        self.loss_weighting: Optional[str] = OB.check_loss_weighting(dm.get("loss_weighting"))
        self.min_snr_gamma: float = OB.check_gamma(dm.get("min_snr_gamma", 5.0))
        # what the network predicts (objective.PREDICTION_TYPES): config['model']['diffusion']['prediction_type'] =
        # "epsilon" (the reference's and the default: everything as without the key), "v_prediction" or "sample".  The training target, the
        # constraint losses' x0^, min_snr's form, every sampler and sampling option follow it.  A plain attribute like the loss keys
        self.prediction_type: str = OB.check_prediction_type(dm.get("prediction_type", "epsilon"))
        # how the mutation block of the output is read: config['model']['diffusion']['mutation_link'] = "identity"
        # (the default: everything as without the key) or "logistic" -- the first mutation_dim outputs are logits of the Bernoulli mean
        # E[x0 | x_t]: cross-entropy in the training step, sigma inside every sampling step and in predict(as_=...).  Needs
        # prediction_type "sample" (ValueError otherwise, here and from every call).  A plain attribute like prediction_type
        self.mutation_link: str = OB.check_mutation_link(dm.get("mutation_link", "identity"), self.prediction_type)
        # differentially private training: None / 0 (the default: today's training call, bit for bit) or the bound C
        # on every row's (patient's) own gradient norm.  A training call with gradients then returns (1/n) sum_r min(1, C / (|g_r| + 1e-6)) g_r;
        # the loss stays the unclipped mean.  train.py's Trainer sets it from training.dp; a plain attribute for users of the bare model.
        # ValueError from the call for what has no per-row gradient (constraint losses, a mixed-up batch source, data parallel)
        self.dp_max_grad_norm: Optional[float] = None
        # training on incomplete patients: None (the default: today's training call, bit for bit) or "mask" --
        # a NaN element of x_0 is "not observed": zero in x_t, left out of the loss and its gradient (MissDiff), the mean still over n D.
        # config['training']['missing_values']; a plain attribute like the loss keys.  ValueError from the call with constraint losses,
        # dp_max_grad_norm, row_sq_error / variational_bound
        self.missing_values: Optional[str] = check_missing_values((config.get("training") or {}).get("missing_values"))
        self._loss_weights = None         # set_loss_weights: a custom per-timestep table (host float32 [T]); wins over loss_weighting
        self._loss_version = 0

    # -- training objective (objective.py) ----------------------------------------
    def set_loss_weights(self, weights=None):
        """Install a custom per-timestep loss-weight table: ``num_steps`` non-negative finite values, gathered by each row's timestep
        (loss = 1/(n D) * sum_r w[t_r] * sum_f rho(d_rf): a mean over n D, not renormalised by the weights).  It takes precedence over
        ``loss_weighting``; ``None`` removes it.  The table is NOT persisted: neither ``state_dict()`` nor the config of a checkpoint
        carries it, so install it again after ``load_trained_model`` (``loss_weighting: min_snr`` is a config key and is restored)."""
        from . import objective as OB
        self._loss_weights = None if weights is None else OB.check_weight_table(weights, self.num_steps)
        self._loss_version += 1

    def _loss_state(self):
        """What the engine's loss setting follows: the objective attributes and the custom table's version counter."""
        return (self.loss_type, self.huber_delta, self.loss_weighting, self.min_snr_gamma, self._loss_version, self.prediction_type)

    # -- constraint losses (north_star; stubs at models/cvae.py:262-302) -----------------------------
    def set_constraints(self, pathways=None, mutation_columns=None, target_columns=None, *, pathway_weight: Optional[float] = None,
                        mutexpr_weight: Optional[float] = None, config: Optional[dict] = None):
        """Add the pathway-coherence and/or mutation-expression terms to the training loss (``forward``).

        pathways: list of member-column lists (columns of the D-wide feature vector; see
        ``constraints.pathways_from_matrix``); mutation_columns / target_columns: the two column sets of the
        correlation block (at most 64 each).  Weights default to ``config['model']['constraints']``
        (config.yaml:57-60) when a config is given, else 1.0.  Call with no arguments to clear."""
        cons = (config or {}).get("model", {}).get("constraints", {})
        if pathways is None and mutation_columns is None:
            self._constraints = None
        else:
            if (mutation_columns is None) != (target_columns is None):
                raise ValueError("mutation_columns and target_columns go together")
            new = {
                "pathways": [list(map(int, p)) for p in (pathways or [])],
                "cols_a": list(map(int, mutation_columns or [])), "cols_b": list(map(int, target_columns or [])),
                "w_pc": float(pathway_weight if pathway_weight is not None else cons.get("pathway_coherence_weight", 1.0)),
                "w_me": float(mutexpr_weight if mutexpr_weight is not None else cons.get("mutation_expression_weight", 1.0)),
            }
            if getattr(self, "feature_transform", None) is not None:
                from .transform import check_transform_training
                check_transform_training(self, new["w_pc"] != 0.0 or new["w_me"] != 0.0)      # ValueError naming data.transform
            self._constraints = new
        self._constraints_version += 1

    def last_row_norms(self, n: int) -> torch.Tensor:
        """|g_r|_2 of the n rows of the most recent training call that ran with ``dp_max_grad_norm`` set: device float32 [n]."""
        eng = self._engine()
        out = torch.empty(int(n), device=eng.device, dtype=torch.float32)
        L.check(L.lib().osd_dp_row_norms(eng.handle, L.ptr(out), int(n)))
        return out

    def last_loss_parts(self):
        """(eps-loss, L_pc, L_me) of the most recent training ``forward`` with constraints configured; the eps-loss is the configured
        one (``loss_type`` / ``loss_weighting``: the MSE by default)."""
        eng = self._engine()
        out = (C.c_float * 3)()
        L.check(L.lib().osd_get_loss_parts(eng.handle, out))
        return float(out[0]), float(out[1]), float(out[2])

    # -- schedule: same torch expressions as models/diffusion.py:312-326, hence bit-identical buffers
    def _get_beta_schedule(self, schedule_type: str, num_steps: int):
        if schedule_type == "linear":
            return torch.linspace(1e-4, 0.02, num_steps)
        if schedule_type == "cosine":
            steps = torch.arange(num_steps + 1, dtype=torch.float32) / num_steps
            abar = torch.cos((steps + 0.008) / 1.008 * np.pi / 2) ** 2
            abar = abar / abar[0]
            return torch.clip(1 - (abar[1:] / abar[:-1]), 0.0001, 0.9999)
        raise ValueError(f"Unknown schedule: {schedule_type}")

    # -- plumbing ---------------------------------------------------------------------------
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engines"] = {}          # device handles are per-process; rebuilt lazily
        return state

    def __deepcopy__(self, memo):
        import copy
        engines, self._engines = self._engines, {}
        try:
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                setattr(new, k, copy.deepcopy(v, memo))
        finally:
            self._engines = engines
        return new

    def _param_list(self):
        return list(self.parameters())

    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def _linked(self) -> bool:
        """Whether the mutation block carries the logistic link; ValueError for an unknown value or a prediction_type other than sample."""
        from . import objective as OB
        return OB.check_mutation_link(getattr(self, "mutation_link", "identity"), self.prediction_type) == "logistic"

    def _refuse_link(self, what: str) -> None:
        """What reads the network's output as x0^ (or folds x0^ away) has no form for a linked model: it is refused, by name."""
        if self._linked():
            raise ValueError(f"{what} is not available with mutation_link 'logistic': it would read the mutation logits as x0^ "
                             f"(set mutation_link to 'identity', or use sample() / predict(as_=...), which carry the link)")

    def _engine(self) -> _Engine:
        linked = self._linked()      # before the device: ValueError for mutation_link / prediction_type that do not go together
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("BiologyAwareDiffusionModel (osteosarcoma_diffusionmodel_amd) runs on MI355X only: "
                               "move the model to a ROCm device (model.to('cuda')); there is no CPU fallback")
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        eng = self._engines.get(key)
        if eng is None:
            with torch.cuda.device(dev):
                eng = _Engine(self, torch.device("cuda", key[1]))
            self._engines[key] = eng
        eng.sync(self)
        if eng.constraints_version != self._constraints_version:
            eng.set_constraints(self._constraints)
            eng.constraints_version = self._constraints_version
        n_link = self.mutation_dim if linked else 0
        if eng.n_link and not n_link:
            eng.set_output_link(0)      # off before the type may leave "sample"
        if eng.prediction_type != self.prediction_type:
            eng.set_prediction(self)    # raises ValueError on an unknown value; the handle then keeps its previous type
            eng.prediction_type = self.prediction_type
        if eng.n_link != n_link:
            eng.set_output_link(n_link)   # on after the type has become "sample"
        state = self._loss_state()
        if eng.loss_state != state:
            eng.set_loss(self)          # raises ValueError on an unknown value; the handle then keeps its previous setting
            eng.loss_state = state
        if eng.dp_clip != float(getattr(self, "dp_max_grad_norm", None) or 0.0):
            eng.set_dp_clip(self)
        mv = getattr(self, "missing_values", None)
        if (mv is not None or eng.loss_mask) and eng.loss_mask != (check_missing_values(mv) == "mask"):
            eng.set_loss_mask(self)     # check_missing_values raises ValueError on an unknown value; the handle then keeps its setting
        for attr, option, encode in ENGINE_OPTIONS:
            value = encode(getattr(self, attr))
            if value is not None:
                L.check(L.lib().osd_set_option(eng.handle, option.encode(), value))
        return eng

    def _prep(self, t: torch.Tensor, cols: Optional[int] = None, name: str = "tensor") -> torch.Tensor:
        dev = self._device()
        if t.device != dev:
            raise RuntimeError(f"{name} is on {t.device} but the model is on {dev}")
        t = t.to(torch.float32).contiguous()
        if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
            raise RuntimeError(f"{name}: expected shape [N, {cols}], got {tuple(t.shape)}")
        return t

    def _t32(self, t: torch.Tensor, n: int, device) -> torch.Tensor:
        """Caller-supplied per-row timestep indices as device int32, range-checked on the host: the reference's
        buffer gather (models/diffusion.py:337) raises IndexError for t outside [0, T).  Costs one sync, only on
        the injected-t path (the default path draws t on the device)."""
        t32 = t.to(device=device, dtype=torch.int32).contiguous()
        if t32.numel() != n:
            raise RuntimeError("t must have one entry per row")
        if n and (int(t32.min()) < 0 or int(t32.max()) >= self.num_steps):
            raise IndexError(f"timestep index out of range [0, {self.num_steps})")
        return t32

    def _note_precision(self, eng) -> None:
        v = C.c_int64(0)
        L.check(L.lib().osd_get_option(eng.handle, b"last_precision", C.byref(v)))
        self.last_precision = "bf16x3" if int(v.value) == 1 else "fp32"

    def _flags(self) -> int:
        return L.OSD_F_TRAIN_MODE if self.training else 0

    def _guidance(self, guidance_scale):
        """(w, c0 as a host float32 array) of a guided call, or None when guidance_scale == 1 (the unguided paths)."""
        w = float(guidance_scale)
        if not np.isfinite(w):
            raise ValueError(f"guidance_scale={guidance_scale} is not finite")
        if np.float32(w) == np.float32(1.0):
            return None
        if self.null_condition is None:
            raise ValueError("guidance_scale != 1 needs the model's null condition: set config['model']['null_condition'] "
                             "(or model.null_condition) to condition_dim floats, the vector condition dropout trained the model on")
        c0 = self.null_condition
        c0 = c0.detach().cpu().numpy() if isinstance(c0, torch.Tensor) else np.asarray(c0)
        c0 = np.ascontiguousarray(c0, dtype=np.float32).reshape(-1)
        if c0.size != self.condition_dim:
            raise ValueError(f"null_condition has {c0.size} entries, condition_dim is {self.condition_dim}")
        if not np.isfinite(c0).all():
            raise ValueError("null_condition is not finite")
        if self.training:
            raise ValueError("guided sampling is eval mode only (model.eval()): no dropout inside a guided evaluation")
        return w, c0

    # -- q_sample (models/diffusion.py:328-342) -------------------------------------------------
    def q_sample(self, x_0, t, noise=None, *, seed: Optional[int] = None, return_target: bool = False):
        """(x_t, noise).  ``return_target=True``: (x_t, target), the training target of the model's ``prediction_type`` as the training
        step forms it -- the noise, a*noise - b*x_0 or x_0."""
        eng = self._engine()
        x_0 = self._prep(x_0, self.data_dim, "x_0")
        n = x_0.shape[0]
        t32 = self._t32(t, n, x_0.device)
        x_t = torch.empty_like(x_0)
        if return_target:
            target = torch.empty_like(x_0)
            if noise is None:
                seed = _draw_seed() if seed is None else seed
            else:
                noise, seed = self._prep(noise, self.data_dim, "noise"), 0
            L.check(L.lib().osd_q_sample_target(eng.handle, L.ptr(x_0), L.ptr(t32), L.ptr(noise), n, seed, 0, L.ptr(x_t), L.ptr(target)))
            return x_t, target
        if noise is None:
            noise_out = torch.empty_like(x_0)
            seed = _draw_seed() if seed is None else seed
            L.check(L.lib().osd_q_sample(eng.handle, L.ptr(x_0), L.ptr(t32), None, n, seed, 0, L.ptr(x_t), L.ptr(noise_out)))
            return x_t, noise_out
        noise = self._prep(noise, self.data_dim, "noise")
        L.check(L.lib().osd_q_sample(eng.handle, L.ptr(x_0), L.ptr(t32), L.ptr(noise), n, 0, 0, L.ptr(x_t), None))
        return x_t, noise

    # -- the per-patient likelihood bound (likelihood.py) ----------------------------
    def _bound_inputs(self, x_0, conditions, what: str):
        if self.training:
            raise ValueError(f"{what} is eval mode only (model.eval()): the bound is a functional of the deterministic network")
        if self.precision == "bf16x3":
            raise ValueError(f"{what} runs on the fp32 kernels: precision='bf16x3' is not accepted")
        x_0 = self._prep(x_0, self.data_dim, "x_0")
        conditions = self._prep(conditions, self.condition_dim, "conditions")
        if conditions.shape[0] != x_0.shape[0]:
            raise RuntimeError(f"conditions has {conditions.shape[0]} rows but x_0 has {x_0.shape[0]}")
        if x_0.shape[0] < 1:
            raise RuntimeError("x_0 has no rows")
        return x_0, conditions

    @torch.no_grad()
    def row_sq_error(self, x_0, conditions, t, *, noise=None, seed: Optional[int] = None, row_offset: int = 0):
        """se [n] (fp32): the squared error sum_d (out - target)^2 of the network's raw output at q_sample(x_0, t) against the training
        target of ``prediction_type``, per row, in eval mode.  ``t``: one timestep index per row.  ``noise`` [n, D] is injected, else
        the draws are generated and keyed by (seed, row_offset + row, t) alone.  Deterministic: the same call returns the same bits.
        ``x_0`` is in model units: with ``feature_transform`` set, ``feature_transform.forward`` of the data."""
        self._refuse_link("row_sq_error")
        x_0, conditions = self._bound_inputs(x_0, conditions, "row_sq_error")
        eng = self._engine()
        n = x_0.shape[0]
        t32 = self._t32(t, n, x_0.device)
        nz = None
        if noise is not None:
            nz = self._prep(noise, self.data_dim, "noise")
            if nz.shape[0] != n:
                raise RuntimeError(f"noise has {nz.shape[0]} rows but x_0 has {n}")
        seed = (0 if nz is not None else _draw_seed()) if seed is None else seed
        se = torch.empty(n, device=x_0.device, dtype=torch.float32)
        L.check(L.lib().osd_row_sq_error(eng.handle, L.ptr(x_0), L.ptr(conditions), n, L.ptr(t32), L.ptr(nz), seed, int(row_offset), L.ptr(se)))
        eng.serial += 1           # the training workspace now belongs to this call
        return se

    def _bound_sweep(self, x_0, conditions, ts, noise, seed, row_offset):
        """se [S][n] (fp32) of osd_bound_sweep over the host int32 array ``ts``."""
        eng = self._engine()
        n, S = x_0.shape[0], int(ts.size)
        nz = None
        if noise is not None:
            if noise.device != x_0.device:
                raise RuntimeError(f"noise is on {noise.device} but the model is on {x_0.device}")
            nz = noise.to(torch.float32).contiguous()
            if tuple(nz.shape) != (S, n, self.data_dim):
                raise RuntimeError(f"noise: expected shape [{S}, {n}, {self.data_dim}], got {tuple(nz.shape)}")
        seed = (0 if nz is not None else _draw_seed()) if seed is None else seed
        se = torch.empty(S, n, device=x_0.device, dtype=torch.float32)
        ts32 = np.ascontiguousarray(ts, dtype=np.int32)
        L.check(L.lib().osd_bound_sweep(eng.handle, L.ptr(x_0), L.ptr(conditions), n, ts32.ctypes.data_as(C.POINTER(C.c_int32)), S, L.ptr(nz),
                                        seed, int(row_offset), L.ptr(se)))
        eng.serial += 1
        return se

    @torch.no_grad()
    def variational_bound(self, x_0, conditions, *, num_timesteps: Optional[int] = None, timesteps=None, noise=None,
                          seed: Optional[int] = None, row_offset: int = 0, decoder_variance: Optional[float] = None):
        """The DDPM's variational upper bound on -log p(x_0 | c) per patient (Ho et al. 2020, eq. 5; likelihood.py states every term).
        ``x_0`` is in model units: with ``feature_transform`` set the bound is a model-space score of ``feature_transform.forward(data)``
        and carries no Jacobian term of the map.

        Returns a dict: ``nll`` [n] in nats and ``bpd`` [n] = nll / (D ln 2), float64 on the device; ``prior`` [n] (L_T, float64);
        ``terms`` [S][n] (float64: row 0 the decoder term L_0, the others the weighted L_t, nll = prior + terms.sum(0));
        ``sq_error`` [S][n], fp32, the raw per-row squared errors of the sweep; ``timesteps`` (int64, ascending, 0 first).

        The default sweeps all ``num_steps`` timesteps: the bound with one draw per term.  ``num_timesteps=S`` takes t = 0 plus
        S - 1 timesteps strided over 1..T-1 and weights their sum by (T - 1)/(S - 1); ``timesteps`` names the set (it must contain 0
        and may not repeat).  ``noise`` [S, n, D] is injected; otherwise the draw of patient ``row_offset + i`` at timestep t depends
        on (seed, that id, t) alone, so a cohort scored in shards, or with another subset containing t, sees the same draw.
        ``decoder_variance``: the variance of the Gaussian decoder of the t = 0 term, by default ``betas[0]`` -- a convention.

        The same functional for every ``prediction_type``, ``loss_type`` and weighting, so checkpoints trained with different
        objectives compare on it.  Mutations are binary, so this continuous density is a RELATIVE score between patients and
        between models, not a calibrated probability.  Eval mode, fp32 kernels (``precision='bf16x3'`` raises ValueError)."""
        from . import likelihood as LK
        from . import objective as OB
        ptype = OB.check_prediction_type(self.prediction_type)
        self._refuse_link("variational_bound")          # no likelihood bound for a Bernoulli block: refused, not approximated
        ts = LK.select_timesteps(self.num_steps, num_timesteps, timesteps)        # ValueError for a bad set, before any device work
        x_0, conditions = self._bound_inputs(x_0, conditions, "variational_bound")
        D, dev = self.data_dim, x_0.device
        w, c0, _ = LK.term_weights(ts, self.betas, self.alphas_cumprod, ptype, D, decoder_variance)      # ValueError for a bad variance
        se = self._bound_sweep(x_0, conditions, ts, noise, seed, row_offset)
        terms = torch.as_tensor(w, dtype=torch.float64, device=dev)[:, None] * se.double()
        terms[0] += c0
        abar = float(self.alphas_cumprod[-1].double())
        prior = 0.5 * (abar * x_0.double().pow(2).sum(1) - D * abar - D * float(np.log1p(-abar)))
        nll = prior + terms.sum(0)
        return {"nll": nll, "bpd": nll / (D * float(np.log(2.0))), "prior": prior, "terms": terms, "sq_error": se,
                "timesteps": torch.as_tensor(ts.astype(np.int64), device=dev)}

    @torch.no_grad()
    def loss_profile(self, x_0, conditions, num_timesteps: int = 50, seed: Optional[int] = None):
        """(timesteps [S] int64, profile [S] float64): the cohort mean of se / D per timestep -- the loss curve of the configured
        target over t -- from the same sweep as ``variational_bound``; ``x_0`` in model units, like there."""
        from . import likelihood as LK
        self._refuse_link("loss_profile")
        ts = LK.select_timesteps(self.num_steps, num_timesteps, None)
        x_0, conditions = self._bound_inputs(x_0, conditions, "loss_profile")
        se = self._bound_sweep(x_0, conditions, ts, None, seed, 0)
        return torch.as_tensor(ts.astype(np.int64), device=x_0.device), se.double().mean(1) / self.data_dim

    # -- training forward (models/diffusion.py:344-380) ------------------------------------------
    def forward(self, x_0, conditions, return_loss=True, *, t=None, noise=None, dropout_masks=None,
                seed: Optional[int] = None):
        from .train import diffusion_loss   # autograd.Function around osd_train_loss_fwd_bwd
        if return_loss:
            return diffusion_loss(self, x_0, conditions, t=t, noise=noise, dropout_masks=dropout_masks, seed=seed)
        # return_loss=False: predicted noise for freshly drawn (or injected) t / noise
        eng = self._engine()
        x_0 = self._prep(x_0, self.data_dim, "x_0")
        conditions = self._prep(conditions, self.condition_dim, "conditions")
        n = x_0.shape[0]
        seed = _draw_seed() if seed is None else seed
        if t is None:
            t = torch.randint(0, self.num_steps, (n,), device=x_0.device)
        x_t, _ = self.q_sample(x_0, t, noise, seed=seed)
        return self._raw_output(x_t, t, conditions, dropout_masks=dropout_masks, seed=seed)      # the raw output, whatever the type

    _AS_KINDS = {"eps": L.OSD_PRED_EPSILON, "v": L.OSD_PRED_V, "x0": L.OSD_PRED_SAMPLE}
    _OWN_AS = {"epsilon": "eps", "v_prediction": "v", "sample": "x0"}

    def predict(self, x_t, t, conditions, as_: str = "raw", *, dropout_masks: Optional[Sequence[torch.Tensor]] = None,
                seed: Optional[int] = None, guidance_scale: float = 1.0):
        """(Model units throughout: a ``feature_transform`` is applied by the generator, never here.)
        The network's prediction at (x_t, t) read as ``as_``: "raw" (the output itself: eps, v or x0 by ``prediction_type``), "x0"
        (x0^ = P x_t + Q out), "eps" ((x_t - a x0^)/b) or "v" (a eps^ - b x0^), a = sqrt_alphas_cumprod[t], b =
        sqrt_one_minus_alphas_cumprod[t].  The conversion is one row-affine pass (osd_convert_prediction) with coefficients formed in float64
        and rounded once; the model's own reading and "raw" are the output unchanged.  ``guidance_scale`` combines raw outputs, which is
        guidance in eps-space for every type.  Conversions are inference only (no autograd through them).

        With ``mutation_link = "logistic"`` "raw" holds logits in the mutation columns; "x0" is sigma of them there (and the output
        elsewhere), "eps" and "v" are derived from that x0^; guidance then acts on the logit in those columns."""
        if as_ != "raw" and as_ not in self._AS_KINDS:
            raise ValueError(f"as_ must be 'raw', 'eps', 'x0' or 'v', got {as_!r}")
        linked = self._linked()
        out = self._raw_output(x_t, t, conditions, dropout_masks=dropout_masks, seed=seed, guidance_scale=guidance_scale)
        from . import objective as OB
        if as_ == "raw" or (not linked and as_ == self._OWN_AS[OB.check_prediction_type(self.prediction_type)]):
            return out
        if out.requires_grad:
            raise ValueError("predict(as_=...) converts without autograd: call it under torch.no_grad(), or use as_='raw'")
        eng = self._engine()
        x_t = self._prep(x_t, self.data_dim, "x_t")
        n = x_t.shape[0]
        t32 = torch.full((n,), int(t), device=x_t.device, dtype=torch.int32) if isinstance(t, int) else self._t32(t, n, x_t.device)
        if isinstance(t, int) and not 0 <= t < self.num_steps:
            raise IndexError(f"timestep index out of range [0, {self.num_steps})")
        L.check(L.lib().osd_convert_prediction(eng.handle, L.ptr(x_t), L.ptr(t32), L.ptr(out), n, self._AS_KINDS[as_], L.ptr(out)))
        return out

    def predict_noise(self, x_t, t, conditions, *, dropout_masks: Optional[Sequence[torch.Tensor]] = None,
                      seed: Optional[int] = None, guidance_scale: float = 1.0):
        """The predicted noise.  An epsilon model: the network's output (``_raw_output``), as ever.  The other types:
        ``predict(as_="eps")``, a real eps^, so that code written against this method (``p_sample`` loops) keeps working.  Model units."""
        if self.prediction_type == "epsilon":
            return self._raw_output(x_t, t, conditions, dropout_masks=dropout_masks, seed=seed, guidance_scale=guidance_scale)
        return self.predict(x_t, t, conditions, "eps", dropout_masks=dropout_masks, seed=seed, guidance_scale=guidance_scale)

    def _raw_output(self, x_t, t, conditions, *, dropout_masks: Optional[Sequence[torch.Tensor]] = None,
                    seed: Optional[int] = None, guidance_scale: float = 1.0):
        """DiffusionUNet.forward(x_t, t/T, condition_embed(c)) (models/diffusion.py:370-373); ``t`` is an
        int (shared) or an integer tensor of per-row timestep indices.

        ``guidance_scale=w`` != 1: the classifier-free-guidance prediction out(c0) + w * (out(c) - out(c0)) with the model's
        ``null_condition`` c0 (eval mode, inference only).  Every type's eps is affine in ``out`` with an x_t term that cancels in the
        difference, so this is guidance in eps-space whatever ``prediction_type`` is."""
        guide = self._guidance(guidance_scale)
        if guide is not None:
            if dropout_masks is not None:
                raise ValueError("guided prediction is eval mode only: no dropout masks")
            if isinstance(x_t, torch.Tensor) and x_t.requires_grad or isinstance(conditions, torch.Tensor) and conditions.requires_grad:
                raise ValueError("guided prediction is inference only: inputs must not require grad")
            eng = self._engine()
            x_t = self._prep(x_t, self.data_dim, "x_t")
            conditions = self._prep(conditions, self.condition_dim, "conditions")
            n = x_t.shape[0]
            if conditions.shape[0] != n:
                raise RuntimeError(f"conditions has {conditions.shape[0]} rows but x_t has {n}")
            eps = torch.empty_like(x_t)
            t_idx, t_all = (None, t) if isinstance(t, int) else (self._t32(t, n, x_t.device), 0)
            L.check(L.lib().osd_denoiser_forward_guided(eng.handle, L.ptr(x_t), L.ptr(t_idx), t_all, L.ptr(conditions), n, L.ptr(eps), 0,
                                                        guide[1].ctypes.data, guide[0]))
            self._note_precision(eng)
            return eps
        eng = self._engine()
        x_t = self._prep(x_t, self.data_dim, "x_t")
        conditions = self._prep(conditions, self.condition_dim, "conditions")
        n = x_t.shape[0]
        eps = torch.empty_like(x_t)
        if isinstance(t, int):
            t_idx, t_all = None, t
        else:
            t_idx, t_all = self._t32(t, n, x_t.device), 0
        flags = self._flags()
        masks = None
        if dropout_masks is not None:
            flags |= L.OSD_F_TRAIN_MODE
            keep = [self._prep(m, name="dropout mask") for m in dropout_masks]
            masks = L.ptr_array(keep)
        seed = _draw_seed() if seed is None else seed
        if torch.is_grad_enabled() and (x_t.requires_grad or any(p.requires_grad for p in self.parameters())):
            # differentiable path (custom losses): activations kept for osd_denoiser_backward
            from .train import denoiser_with_grad
            if t_idx is None:
                t_idx = torch.full((n,), t_all, device=x_t.device, dtype=torch.int32)
            self.last_precision = "fp32"          # the differentiable path keeps the activations of the fp32 kernels
            return denoiser_with_grad(self, x_t, t_idx, conditions, keep if dropout_masks is not None else None, seed, flags)
        L.check(L.lib().osd_denoiser_forward(eng.handle, L.ptr(x_t), L.ptr(t_idx), t_all, L.ptr(conditions), n,
                                             L.ptr(eps), flags, masks, seed))
        self._note_precision(eng)
        return eps

    # -- p_sample / sample (models/diffusion.py:382-449) ------------------------------------------
    @torch.no_grad()
    def p_sample(self, x_t, t, conditions, *, noise=None, seed: Optional[int] = None):
        """One reverse step, in model units (a ``feature_transform`` is applied by the generator, never here)."""
        self._refuse_link("p_sample")       # the single step folds x0^ away; sample() runs the x0-unfolded steps
        eng = self._engine()
        x_t = self._prep(x_t, self.data_dim, "x_t")
        conditions = self._prep(conditions, self.condition_dim, "conditions")
        n = x_t.shape[0]
        out = torch.empty_like(x_t)
        z = None if noise is None else self._prep(noise, self.data_dim, "noise")
        seed = _draw_seed() if (seed is None and z is None) else (seed or 0)
        L.check(L.lib().osd_p_sample_step(eng.handle, L.ptr(x_t), int(t), L.ptr(conditions), L.ptr(z), n, seed, 0,
                                          L.ptr(out), self._flags()))
        self._note_precision(eng)
        return out

    @torch.no_grad()
    def sample(self, conditions, num_samples: int = 1, *, x_T=None, noise=None, seed: Optional[int] = None,
               row_offset: int = 0, return_mutation_mask: bool = False, num_inference_steps: Optional[int] = None,
               eta: float = 0.0, guidance_scale: float = 1.0, known=None, x0_bounds=None, solver: Optional[str] = None,
               timestep_spacing: str = "uniform", timesteps=None, _step_plan=None):
        """Full reverse chain, in MODEL units: with ``feature_transform`` set the samples, ``known`` and ``x0_bounds`` are what
        ``feature_transform.forward`` makes of data (``SyntheticPatientGenerator`` speaks data units and maps both ways).
        ``x_T`` [N,D] and ``noise`` [T-1,N,D] (draw order t = T-1..1) inject the
        random draws; otherwise Philox(seed, row_offset + row) generates them on the device.

        ``num_inference_steps=S`` runs the strided DDIM sampler instead (ddim.py: S of the T timesteps, ``eta`` in [0, 1]
        scales its noise; 0 is deterministic after x_T, 1 with S = T is the DDPM chain).  x_T is the DDPM chain's for the same
        seed / row_offset; ``noise`` is then [S-1,N,D] (draw order s = S-1..1) and needs eta > 0.

        ``guidance_scale=w`` != 1 runs the classifier-free-guidance chain (DDPM or DDIM alike): every step uses
        eps(c0) + w * (eps(c) - eps(c0)), c0 the model's ``null_condition``; the draws are the unguided chain's.  Per-layer kernels
        (``last_sampler == "graph"``), fp32, eval mode.

        ``known`` [N,D] samples around observed values (the replacement method): a finite element is an observation and comes
        back exactly, NaN leaves the element to the chain (Inf raises ValueError).  After every step the observed elements are
        overwritten with the observation noised to the level the state has reached, sqrt(abar')*known + sqrt(1 - abar')*z, z the
        step's own draw at that element -- so ``noise`` is accepted at eta = 0 too, where it feeds only the observed elements.
        Works with the DDPM chain, ``num_inference_steps`` / ``eta`` and ``guidance_scale``; per-layer kernels
        (``last_sampler == "graph"``), fp32.  ``known=None`` or all-NaN is the unconstrained call.

        ``x0_bounds`` clips the predicted clean sample x0^ = P x + Q out of every step -- (x - sqrt(1-abar) out)/sqrt(abar) for an epsilon
        model, sqrt(abar) x - sqrt(1-abar) out for v_prediction, out for sample -- to per-feature bounds before
        the posterior update (clip_denoised / clip_sample elsewhere), the direction term using the eps the clipped x0^ implies: a
        ``(lo, hi)`` pair of scalars or [D] arrays, or a dict over ``mutations`` / ``expression`` / ``pathways`` of such pairs
        (``generate.assemble_bounds``; a missing block or a ``None`` side is free).  Every returned element lies inside its bounds
        exactly -- except observed elements of ``known``, which come back as observed.  ``None`` takes ``model.x0_bounds`` (``None`` by
        default: no clipping, today's entry points on any engine, the same bits); ``False`` ignores the attribute.  Works with the DDPM
        chain, ``num_inference_steps`` / ``eta``, ``guidance_scale`` and ``known``; per-layer kernels (``last_sampler == "graph"``), fp32
        (``precision = "bf16x3"`` raises ValueError).

        The chain follows ``prediction_type``: every step is x' = E x0^ + F x + C z with x0^ = P x + Q out, and only (P, Q) depend on the
        type, so every engine and every option above runs a v_prediction or sample model from refolded tables, at the same speed.

        ``solver`` is ``None`` or ``"ddim"`` (the calls above, any engine, the same bits) or ``"dpmpp_2m"``: DPM-Solver++(2M) (Lu et al.
        2022), the second-order multistep solver on the predicted x0^ -- the eta = 0 DDIM step plus one term in the previous step's clipped
        x0^ (``ddim.dpmpp_2m_table``), inside the same launch.  It needs ``num_inference_steps`` and ``eta == 0``, takes ``noise`` only
        together with ``known`` (whose observed elements it feeds), and runs with ``guidance_scale``, ``known``, ``x0_bounds`` and every
        ``prediction_type``; per-layer kernels (``last_sampler == "graph"``), fp32 (``precision = "bf16x3"`` raises ValueError).

        ``timestep_spacing`` chooses the S timesteps of ``num_inference_steps``, for either solver: ``"uniform"`` (``ddim.ddim_timesteps``)
        or ``"logsnr"`` (``ddim.logsnr_timesteps``: uniform in ln(sqrt(abar)/sqrt(1-abar)); better for the multistep solver from about ten
        steps on, worse for DDIM and at five).  Without ``num_inference_steps`` it must be ``"uniform"``.

        ``mutation_link = "logistic"``: the mutation columns of the output are logits, and every step takes
        x0^ = sigma(out) there before the clamp, so every returned mutation value lies in [0, 1] with no ``x0_bounds`` given.  Such a model
        always runs the x0-unfolded steps -- the ``x0_bounds`` path with infinite bounds where none are given, or ``solver="dpmpp_2m"`` --
        whatever the other options are: per-layer kernels (``last_sampler == "graph"``), fp32 (``precision = "bf16x3"`` raises
        ValueError).  ``guidance_scale`` combines raw outputs, so on the mutation columns it acts in logit space.

        ``timesteps`` names the plan itself -- strictly increasing timestep indices, e.g. the ``timesteps`` of an ``invert`` record -- in
        place of one derived from ``num_inference_steps`` and ``timestep_spacing``, which are then not used: ``x_T`` is the state at
        ``timesteps[-1]`` and ``noise`` is [len(timesteps)-1, N, D].  Every option above keeps its meaning.  ``None`` keeps every path
        above and its bits."""
        from . import objective as OB
        pred = OB.check_prediction_type(self.prediction_type)
        linked = self._linked()
        if linked and self.precision == "bf16x3":
            raise ValueError("mutation_link 'logistic' samples on the fp32 kernels: precision='bf16x3' is not accepted")
        sched = dict(sqrt_alphas_cumprod=self.sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod=self.sqrt_one_minus_alphas_cumprod)
        guide = self._guidance(guidance_scale)
        if solver not in (None, "ddim", "dpmpp_2m"):
            raise ValueError(f"solver must be None, 'ddim' or 'dpmpp_2m', got {solver!r}")
        if timestep_spacing not in ("uniform", "logsnr"):
            raise ValueError(f"timestep_spacing must be 'uniform' or 'logsnr', got {timestep_spacing!r}")
        multistep = solver == "dpmpp_2m"
        taus = None
        if timesteps is not None:
            taus = np.asarray(timesteps.detach().cpu().numpy() if isinstance(timesteps, torch.Tensor) else timesteps).reshape(-1)
            if taus.size < 1 or not np.issubdtype(taus.dtype, np.integer):
                raise ValueError("timesteps must be a non-empty list of integer timestep indices")
            if int(taus.min()) < 0 or int(taus.max()) >= self.num_steps or not (np.diff(taus.astype(np.int64)) > 0).all():
                raise ValueError(f"timesteps must strictly increase inside [0, {self.num_steps})")
            taus = taus.astype(np.int32)
            num_inference_steps = int(taus.size)
        if _step_plan is not None:          # invert(method="ddim"): the rows are given, not derived
            num_inference_steps = int(_step_plan[0].size)
        if num_inference_steps is None:
            if multistep:
                raise ValueError("solver='dpmpp_2m' needs num_inference_steps")
            if timestep_spacing != "uniform":
                raise ValueError("timestep_spacing applies to num_inference_steps: pass it as well")
        if multistep and float(eta) != 0.0:
            raise ValueError("solver='dpmpp_2m' is deterministic: eta must be 0")
        if x0_bounds is None:
            x0_bounds = self.x0_bounds
        bounds = None
        if x0_bounds is not None and x0_bounds is not False:
            from .generate import assemble_bounds
            bounds = assemble_bounds(x0_bounds, self.mutation_dim, self.expression_dim, self.pathway_dim)
        elif linked:
            # the x0-unfolded steps carry the link: all columns free (sigma itself keeps the mutation block inside [0, 1])
            bounds = (np.full(self.data_dim, -np.inf, dtype=np.float32), np.full(self.data_dim, np.inf, dtype=np.float32))
        kn = None
        if known is not None:
            kn = self._prep(known, self.data_dim, "known")
            if kn.shape[0] != int(num_samples):
                raise RuntimeError(f"known has {kn.shape[0]} rows but num_samples is {int(num_samples)}")
            if bool(torch.isinf(kn).any()):
                raise ValueError("known holds Inf: an observation is finite, NaN marks a free element")
            if bool(torch.isnan(kn).all()):
                kn = None                       # nothing observed: today's entry points, any engine, their bits
        plan = None
        if num_inference_steps is not None:
            from .ddim import ddim_step_table, ddim_timesteps, dpmpp_2m_table, logsnr_timesteps
            if not 0.0 <= float(eta) <= 1.0:
                raise ValueError(f"eta={eta} outside [0, 1]")
            steps = int(num_inference_steps)
            if not 1 <= steps <= self.num_steps:
                raise ValueError(f"num_inference_steps={steps} outside [1, {self.num_steps}]")
            if noise is not None and float(eta) == 0.0 and kn is None:
                raise ValueError("noise: eta = 0 draws no z (pass eta > 0 or leave noise out)")
            if taus is None:
                taus = ddim_timesteps(self.num_steps, steps) if timestep_spacing == "uniform" else logsnr_timesteps(self.alphas_cumprod, steps)
            if _step_plan is not None:
                plan = _step_plan
            elif multistep:
                plan = dpmpp_2m_table(self.alphas_cumprod, taus, pred, **sched)
            else:
                plan = ddim_step_table(self.alphas_cumprod, taus, eta, pred, **sched)
        elif float(eta) != 0.0:
            raise ValueError("eta applies to the DDIM sampler: pass num_inference_steps as well")
        n_draws = self.num_steps - 1 if plan is None else plan[0].size - 1
        eng = self._engine()
        conditions = self._prep(conditions, self.condition_dim, "conditions")
        n = int(num_samples)
        if conditions.shape[0] != n:
            # the reference broadcasts-or-fails here (models/diffusion.py:443-447)
            raise RuntimeError(f"conditions has {conditions.shape[0]} rows but num_samples is {n}")
        out = torch.empty(n, self.data_dim, device=conditions.device, dtype=torch.float32)
        xT = None if x_T is None else self._prep(x_T, self.data_dim, "x_T")
        zs = None
        if noise is not None:
            zs = noise.to(torch.float32).contiguous()
            if tuple(zs.shape) != (n_draws, n, self.data_dim):
                raise RuntimeError(f"noise: expected shape [{n_draws}, {n}, {self.data_dim}]")
        mask = torch.empty(n, self.mutation_dim, device=out.device, dtype=torch.float32) if return_mutation_mask else None
        if seed is None:
            seed = _draw_seed()
        flags = self._flags() | (L.OSD_F_GRAPH if self.use_graph else 0)
        engine = 0 if (guide is not None or kn is not None or bounds is not None or multistep) else L.lib().osd_sample_engine(eng.handle, n, flags)
        if engine < 0:
            L.check(engine)
        if engine == 1:
            # the chain kernel's bounded waits report through a status word: the synchronous call reads it and, should the
            # chain have given up, re-runs it on the per-layer kernels (same bits) -- sample() cannot fail, as the reference's
            flags |= L.OSD_F_SYNC

        def counter(name):
            v = C.c_int64(0)
            L.check(L.lib().osd_get_option(eng.handle, name, C.byref(v)))
            return int(v.value)

        gave_up_before = counter(b"chain_fallbacks")
        if multistep:
            from .ddim import known_level_table
            tau, x0c, hist = plan
            level = None if kn is None else known_level_table(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, tau)
            L.check(L.lib().osd_sample_chain_multistep(eng.handle, L.ptr(conditions), n, L.ptr(xT), L.ptr(zs), seed, int(row_offset),
                                                       L.ptr(out), L.ptr(mask), flags, tau.ctypes.data, x0c.ctypes.data, hist.ctypes.data,
                                                       None if level is None else level.ctypes.data, int(tau.size),
                                                       None if guide is None else guide[1].ctypes.data, 1.0 if guide is None else guide[0],
                                                       L.ptr(kn), self.data_dim, None if bounds is None else bounds[0].ctypes.data,
                                                       None if bounds is None else bounds[1].ctypes.data))
        elif bounds is not None:
            from .ddim import ddim_x0_table, known_level_table
            tau, coef = plan if plan is not None else (None, None)
            x0c = None if tau is None else ddim_x0_table(self.alphas_cumprod, tau, eta, pred, **sched)
            level = None
            if tau is not None and kn is not None:
                level = known_level_table(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, tau)
            L.check(L.lib().osd_sample_chain_clipped(eng.handle, L.ptr(conditions), n, L.ptr(xT), L.ptr(zs), seed, int(row_offset),
                                                     L.ptr(out), L.ptr(mask), flags, None if tau is None else tau.ctypes.data,
                                                     None if coef is None else coef.ctypes.data, None if x0c is None else x0c.ctypes.data,
                                                     None if level is None else level.ctypes.data, 0 if tau is None else int(tau.size),
                                                     None if guide is None else guide[1].ctypes.data, 1.0 if guide is None else guide[0],
                                                     L.ptr(kn), self.data_dim, bounds[0].ctypes.data, bounds[1].ctypes.data))
        elif kn is not None:
            from .ddim import known_level_table
            tau, coef = plan if plan is not None else (None, None)
            level = None if tau is None else known_level_table(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, tau)
            L.check(L.lib().osd_sample_chain_known(eng.handle, L.ptr(conditions), n, L.ptr(xT), L.ptr(zs), seed, int(row_offset),
                                                   L.ptr(out), L.ptr(mask), flags, None if tau is None else tau.ctypes.data,
                                                   None if coef is None else coef.ctypes.data,
                                                   None if level is None else level.ctypes.data, 0 if tau is None else int(tau.size),
                                                   None if guide is None else guide[1].ctypes.data, 1.0 if guide is None else guide[0],
                                                   L.ptr(kn), self.data_dim))
        elif guide is not None:
            tau, coef = plan if plan is not None else (None, None)
            L.check(L.lib().osd_sample_chain_guided(eng.handle, L.ptr(conditions), n, L.ptr(xT), L.ptr(zs), seed, int(row_offset),
                                                    L.ptr(out), L.ptr(mask), flags, None if tau is None else tau.ctypes.data,
                                                    None if coef is None else coef.ctypes.data, 0 if tau is None else int(tau.size),
                                                    guide[1].ctypes.data, guide[0]))
        elif plan is None:
            L.check(L.lib().osd_sample_chain(eng.handle, L.ptr(conditions), n, L.ptr(xT), L.ptr(zs), seed, int(row_offset),
                                             L.ptr(out), L.ptr(mask), flags))
        else:
            tau, coef = plan
            L.check(L.lib().osd_sample_chain_steps(eng.handle, L.ptr(conditions), n, L.ptr(xT), L.ptr(zs), seed, int(row_offset),
                                                   L.ptr(out), L.ptr(mask), flags, tau.ctypes.data, coef.ctypes.data, int(tau.size)))
        used = L.lib().osd_sample_engine(eng.handle, -1, 0)      # the engine that produced the result
        if used < 0:
            L.check(used)
        self.last_sampler = "chain" if used == 1 else "graph"
        self._note_precision(eng)
        # a chain kernel ran iff the result is its own or it gave up and was re-run (the counter moved); a call the library
        # demoted up front (injected draws at D % 4 != 0 keep the guarded per-layer kernels) launched none and warns about nothing
        gave_up = counter(b"chain_fallbacks") > gave_up_before
        self.last_chain_variant = self.last_squad_panel = None
        if used == 1 or gave_up:
            self.last_chain_variant = {1: "workspace", 2: "panel", 3: "squad"}.get(counter(b"last_chain_variant"))
            self.last_squad_panel = counter(b"last_squad_panel") if self.last_chain_variant == "squad" else None
        if gave_up:
            import warnings
            warnings.warn(L.last_error() or "the reverse-chain kernel gave up; the chain was re-run on the per-layer kernels")
        if return_mutation_mask:
            return out, mask
        return out

    # -- counterfactual patients: inversion and edit ---------------------------------
    @torch.no_grad()
    def invert(self, x_0, conditions, *, method: str = "ddpm", num_inference_steps: int = 50, strength: float = 1.0, eta: float = 1.0,
               timestep_spacing: str = "uniform", noise=None, seed: Optional[int] = None, row_offset: int = 0) -> "Inversion":
        """Turn patients ``x_0`` [N, D] (model units) under ``conditions`` into what ``sample`` turns back into them: an ``Inversion``
        record (``timesteps``, ``x_start``, ``noise``, ``eta``, ``method``).  ``sample(conditions, N, x_T=rec.x_start, noise=rec.noise,
        timesteps=rec.timesteps, eta=rec.eta)`` replays it; under other conditions it is the counterfactual (``edit`` does both).

        The levels are ``ddim.edit_timesteps``: the first ``round(strength * num_inference_steps)`` timesteps of the plan, timestep 0 in
        front -- ``strength`` in (0, 1] is how far up the patient is noised, i.e. how much of it the edit may change.

        ``method="ddpm"``: the edit-friendly DDPM noise space (Huberman-Spiegelglas et al. 2024), one ``osd_noise_map`` call.  The patient
        is noised independently to every level (``noise`` [S, N, D] injects those draws; otherwise they are keyed by (seed, row_offset +
        row, timestep) alone) and every step of the plan is solved for the draw that carries one level's state to the next, so the
        replay reconstructs the patient by construction: it returns the model's x0^ at ``timesteps[0]`` from a state one tiny step
        above the patient.  Needs ``eta`` > 0; eval mode, fp32 kernels.  ``rec.noise`` is [S-1, N, D].

        ``method="ddim"``: DDIM inversion (Song et al. 2021), the eta = 0 step run upwards (``ddim.ddim_inversion_table``) from the
        patient as the state at ``timesteps[0]``: one ``osd_sample_chain_steps`` call on any engine (``last_sampler`` says which).
        ``rec.noise`` is None and ``rec.eta`` 0; ``eta``, ``noise`` and ``seed`` are not used.

        Inversion is always unguided and unclipped.  ValueError: ``method="ddpm"`` with ``eta <= 0`` or ``precision="bf16x3"``,
        ``strength`` outside (0, 1], a ``mutation_link`` model (its step is not the affine row either method inverts)."""
        from . import objective as OB
        from .ddim import ddim_inversion_table, ddim_step_table, edit_timesteps
        if method not in ("ddpm", "ddim"):
            raise ValueError(f"method must be 'ddpm' or 'ddim', got {method!r}")
        pred = OB.check_prediction_type(self.prediction_type)
        self._refuse_link("invert")
        if timestep_spacing not in ("uniform", "logsnr"):
            raise ValueError(f"timestep_spacing must be 'uniform' or 'logsnr', got {timestep_spacing!r}")
        steps = int(num_inference_steps)
        if not 1 <= steps <= self.num_steps:
            raise ValueError(f"num_inference_steps={steps} outside [1, {self.num_steps}]")
        levels = edit_timesteps(self.num_steps, steps, strength, self.alphas_cumprod, timestep_spacing)
        sched = dict(sqrt_alphas_cumprod=self.sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod=self.sqrt_one_minus_alphas_cumprod)
        if method == "ddpm":
            if not 0.0 < float(eta) <= 1.0:
                raise ValueError(f"method='ddpm' solves every step for its draw and needs eta in (0, 1], got eta={eta}")
            if self.precision == "bf16x3":
                raise ValueError("invert(method='ddpm') runs on the fp32 kernels: precision='bf16x3' is not accepted")
        if self.training:
            raise ValueError("invert is eval mode only (model.eval()): it inverts the deterministic network")
        x_0 = self._prep(x_0, self.data_dim, "x_0")
        conditions = self._prep(conditions, self.condition_dim, "conditions")
        n = x_0.shape[0]
        if conditions.shape[0] != n:
            raise RuntimeError(f"conditions has {conditions.shape[0]} rows but x_0 has {n}")
        if n < 1:
            raise RuntimeError("x_0 has no rows")
        if method == "ddim":
            plan = ddim_inversion_table(self.alphas_cumprod, levels, pred, **sched)
            x_start = self.sample(conditions, n, x_T=x_0, seed=0, x0_bounds=False, _step_plan=plan)
            return Inversion(levels, x_start, None, 0.0, "ddim")
        tau, coef = ddim_step_table(self.alphas_cumprod, levels, eta, pred, **sched)
        S = int(tau.size)
        eng = self._engine()
        nz = None
        if noise is not None:
            if noise.device != x_0.device:
                raise RuntimeError(f"noise is on {noise.device} but the model is on {x_0.device}")
            nz = noise.to(torch.float32).contiguous()
            if tuple(nz.shape) != (S, n, self.data_dim):
                raise RuntimeError(f"noise: expected shape [{S}, {n}, {self.data_dim}], got {tuple(nz.shape)}")
        seed = (0 if nz is not None else _draw_seed()) if seed is None else seed
        x_start = torch.empty_like(x_0)
        zs = torch.empty(S - 1, n, self.data_dim, device=x_0.device, dtype=torch.float32)
        L.check(L.lib().osd_noise_map(eng.handle, L.ptr(x_0), L.ptr(conditions), n, tau.ctypes.data, coef.ctypes.data, S, L.ptr(nz), seed,
                                      int(row_offset), L.ptr(x_start), L.ptr(zs) if S > 1 else None))
        eng.serial += 1           # the training workspace now belongs to this call
        self.last_precision = "fp32"
        return Inversion(levels, x_start, zs, float(eta), "ddpm")

    @torch.no_grad()
    def edit(self, x_0, conditions, new_conditions, *, method: str = "ddpm", num_inference_steps: int = 50, strength: float = 1.0,
             eta: float = 1.0, timestep_spacing: str = "uniform", noise=None, seed: Optional[int] = None, row_offset: int = 0,
             guidance_scale: float = 1.0, x0_bounds=None, known=None):
        """The counterfactual of patients ``x_0`` [N, D]: ``invert`` under ``conditions``, then ``sample`` under ``new_conditions`` from
        the record -- what the model makes of the same patients' noise under another condition.  Model units, like ``sample``.

        The inversion is always unguided and unclipped; ``guidance_scale``, ``x0_bounds`` and ``known`` (``sample``'s meanings: e.g. hold
        the observed mutations) apply to the decode, through the guided, clipped and known chains with the record's draws.  With
        ``new_conditions`` equal to ``conditions`` and ``method="ddpm"`` the result is the model's own x0^ of the patient at level 0."""
        rec = self.invert(x_0, conditions, method=method, num_inference_steps=num_inference_steps, strength=strength, eta=eta,
                          timestep_spacing=timestep_spacing, noise=noise, seed=seed, row_offset=row_offset)
        n = rec.x_start.shape[0]
        zs = rec.noise if rec.noise is not None and rec.noise.shape[0] > 0 else None
        return self.sample(new_conditions, n, x_T=rec.x_start, noise=zs, seed=0, row_offset=row_offset, eta=rec.eta,
                           guidance_scale=guidance_scale, known=known, x0_bounds=x0_bounds, timesteps=rec.timesteps)


class Inversion:
    """What ``BiologyAwareDiffusionModel.invert`` returns: ``timesteps`` (int32 numpy, increasing, the plan ``sample(timesteps=...)``
    replays), ``x_start`` [N, D] (the state at ``timesteps[-1]``), ``noise`` [len(timesteps)-1, N, D] in the chain's draw order (None for
    ``"ddim"``), ``eta`` and ``method``."""
    __slots__ = ("timesteps", "x_start", "noise", "eta", "method")

    def __init__(self, timesteps, x_start, noise, eta, method):
        self.timesteps, self.x_start, self.noise, self.eta, self.method = timesteps, x_start, noise, eta, method

    def __repr__(self):
        return (f"Inversion(method={self.method!r}, eta={self.eta}, timesteps={self.timesteps.tolist()}, "
                f"x_start={tuple(self.x_start.shape)}, noise={None if self.noise is None else tuple(self.noise.shape)})")


# north_star alias (there is no class of this name in the reference)
BiologyAwareDiffusion = BiologyAwareDiffusionModel
