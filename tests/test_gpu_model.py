"""GPU: BiologyAwareDiffusionModel / SyntheticPatientGenerator (HIP path through the C ABI)
against the golden fixtures the reference produced and against the CPU oracle.

Stated fp32 tolerances (BASELINE.md parity gate):
  single op / single step   max|d| <= 1e-5 * max|ref|
  full reverse chain        max|d| <= 5e-5 * max|ref|
  mutation mask             bit-exact as an operation on the sampler output; mismatches vs the
                            reference reported and required to be 0 except within tolerance of 0.5
"""
import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusion, BiologyAwareDiffusionModel, SyntheticPatientGenerator
from osteosarcoma_diffusionmodel_amd import generate_patients
from helpers import (FULL, FULL_H, SM, SM_H, assert_close, config, golden_small_sd, load_golden, small_model)

pytestmark = pytest.mark.gpu
STEP_RTOL, CHAIN_RTOL = 1e-5, 5e-5


def dev(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def test_state_dict_contract(golden_dir):
    m = BiologyAwareDiffusionModel(config=config(SM_H), **SM)
    sd = golden_small_sd(golden_dir)
    assert list(m.state_dict().keys()) == list(sd.keys())            # names and order of the reference
    assert all(m.state_dict()[k].shape == v.shape for k, v in sd.items())
    bufs = O.schedule_buffers("cosine", 1000)
    for k in ("betas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
        assert torch.equal(m.state_dict()[k], bufs[k])                # same expressions, same host: bit-identical
        # vs the reference's buffers generated on another host CPU: torch's vectorised cos differs in the last bit
        assert_close(m.state_dict()[k], sd[k], 1e-6, what=k)
    assert BiologyAwareDiffusion is BiologyAwareDiffusionModel
    assert not hasattr(m, "vae")                                      # Trainer dispatch, utils/train.py:233
    with pytest.raises(ValueError):
        BiologyAwareDiffusionModel(config=config(SM_H, schedule="sigmoid"), **SM)


def test_eval_forward_small(golden_dir):
    g = load_golden(golden_dir, "g3g4_small_model")
    m = small_model(golden_dir)
    eps = m.predict_noise(dev(g["x"]), dev(g["t"]), dev(g["cond"]))
    assert_close(eps.cpu(), g["eval_noise_pred"], STEP_RTOL, what="noise_pred vs reference")


def test_q_sample_bit_exact(golden_dir):
    g = load_golden(golden_dir, "g3g4_small_model")
    m = small_model(golden_dir)
    x_t, noise = m.q_sample(dev(g["x"]), dev(g["t"]), dev(g["noise"]))
    assert_close(x_t.cpu(), g["q_sample_x_t"], 1e-6, what="q_sample vs reference")
    bufs = {k: v.cpu() for k, v in m.state_dict().items() if "alpha" in k or k == "betas"}
    ref = O.q_sample(bufs, torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g["noise"]))
    assert np.array_equal(x_t.cpu().numpy(), ref.numpy())            # bit-exact given the same schedule buffers
    assert np.array_equal(noise.cpu().numpy(), g["noise"])
    # generated noise: standard normal, returned alongside x_t
    x0 = torch.zeros(2048, 40, device="cuda")
    x_t, noise = m.q_sample(x0, torch.full((2048,), 999, device="cuda"), seed=3)
    assert abs(float(noise.mean())) < 0.02 and abs(float(noise.var()) - 1) < 0.03
    assert_close(x_t.cpu(), (m.sqrt_one_minus_alphas_cumprod[999] * noise).cpu(), 1e-6)


def test_train_mode_forward_with_masks(golden_dir):
    """Dropout keep-masks injected: forward in train mode equals the reference's train-mode forward."""
    g = load_golden(golden_dir, "g3g4_small_model")
    m = small_model(golden_dir)
    sd = {k: v for k, v in golden_small_sd(golden_dir).items() if k.startswith(("condition_embed", "unet"))}
    bufs = O.schedule_buffers("cosine", 1000)
    x, cond, t, noise = (torch.from_numpy(g[k]) for k in ("x", "cond", "t", "noise"))
    masks = [torch.from_numpy(g[f"train_mask.{i}"]) for i in range(5)]
    ref = O.training_forward(sd, bufs, x, cond, t, noise, 3, 128, masks, 0.2, return_loss=False)
    x_t, _ = m.q_sample(x.cuda(), t.cuda(), noise.cuda())
    eps = m.predict_noise(x_t, t.cuda(), cond.cuda(), dropout_masks=[k.cuda() for k in masks])
    assert_close(eps.cpu(), ref, STEP_RTOL, what="train-mode forward")


def test_p_sample_steps(golden_dir):
    g = load_golden(golden_dir, "g5_sampling")
    m = small_model(golden_dir)
    x_t, cond = dev(g["step_x_t"]), dev(g["cond"])
    for t in (999, 998, 500, 1, 0):
        y = m.p_sample(x_t, t, cond, noise=dev(g[f"step_{t}_z"]))
        assert_close(y.cpu(), g[f"step_{t}_out"], STEP_RTOL, what=f"p_sample t={t}")


@pytest.mark.parametrize("T", [50, 1000])
@pytest.mark.parametrize("graph", [False, True])
def test_full_chain_vs_reference(golden_dir, T, graph):
    g = load_golden(golden_dir, "g5_sampling")
    m = small_model(golden_dir, T=T)
    m.use_graph = graph
    out, mask = m.sample(dev(g["cond"]), 3, x_T=dev(g[f"chain_{T}_x_T"]), noise=dev(g[f"chain_{T}_z"]),
                         return_mutation_mask=True)
    ref = g[f"chain_{T}_out"]
    assert_close(out.cpu(), ref, CHAIN_RTOL, what=f"chain T={T}")
    got = out.cpu().numpy()
    assert np.array_equal(mask.cpu().numpy(), (got[:, :8] > 0.5).astype(np.float32))      # bit-exact as an op
    near = np.abs(ref[:, :8] - 0.5) <= CHAIN_RTOL * np.abs(ref).max()
    mism = (mask.cpu().numpy() != g[f"chain_{T}_mut_mask"]) & ~near
    assert mism.sum() == 0, f"{mism.sum()} mutation-mask mismatches vs the reference"


def test_generate_dict_vs_reference(golden_dir):
    g = load_golden(golden_dir, "g7_generation")
    m = small_model(golden_dir, T=20)
    conf = config(SM_H, T=20)
    gen = SyntheticPatientGenerator(m, conf, device="cuda")
    scen = dict(survival_time=300, event_occurred=1, metastasis_at_diagnosis=1)
    res = gen.generate(6, scen, x_T=dev(g["gen_x_T"]), noise=dev(g["gen_z"]))
    assert set(res) == {"mutations", "expression", "pathways", "conditions"}
    assert res["mutations"].dtype == np.float64 and set(np.unique(res["mutations"])) <= {0.0, 1.0}
    assert np.array_equal(res["conditions"], g["gen.conditions"])
    assert_close(res["expression"], g["gen.expression"], CHAIN_RTOL)
    assert_close(res["pathways"], g["gen.pathways"], CHAIN_RTOL)
    assert np.array_equal(res["mutations"], g["gen.mutations"])
    # create_conditions: pad / truncate with a warning, never an error (utils/generate.py:76-82)
    for cd in (4, 2):
        mm = BiologyAwareDiffusionModel(8, 24, 8, cd, conf)
        gg = SyntheticPatientGenerator(mm, conf, device="cuda")
        for name, s in (("early_stage_good_prognosis", dict(survival_time=2000, event_occurred=0, metastasis_at_diagnosis=0)),
                        ("typical_patient", dict(survival_time=800, event_occurred=0, metastasis_at_diagnosis=0))):
            assert np.array_equal(gg.create_conditions(5, s).cpu().numpy(), g[f"cd{cd}.{name}"])
    assert gen.create_conditions(7).shape == (7, 3)
    out = generate_patients(m, conf, 5, scen, seed=1)
    assert out["expression"].shape == (5, 24)


def full_model(seed):
    shapes = O.param_shapes(50, 1900, 50, 3, FULL_H, 128)
    sd = O.init_state_dict(shapes, seed=seed)
    m = BiologyAwareDiffusionModel(config=config(FULL_H), **FULL)
    m.load_state_dict(sd, strict=False)
    return m.cuda().eval(), sd


def test_full_shape_vs_reference(golden_dir):
    g = load_golden(golden_dir, "g8_full_shape")
    m, _ = full_model(int(g["init_seed"]))
    eps = m.predict_noise(dev(g["x"]), dev(g["t"]), dev(g["cond"]))
    assert_close(eps.cpu(), g["noise_pred"], STEP_RTOL, what="D=2000 noise_pred")
    y = m.p_sample(dev(g["x"]), 640, dev(g["cond"]), noise=dev(g["z"]))
    assert_close(y.cpu(), g["p_sample_640"], STEP_RTOL, what="D=2000 p_sample")


def test_full_shape_chain_vs_oracle():
    """D=2000, T=1000, 40 rows with the device's own Philox noise: the oracle replays the chain
    on the host with the identical noise (read back through osd_op_randn)."""
    import ctypes as C
    from osteosarcoma_diffusionmodel_amd import _lib as L
    m, sd = full_model(11)
    n, D, T, seed = 40, 2000, 1000, 4242
    cond = torch.randn(n, 3, generator=torch.Generator().manual_seed(1))
    out = m.sample(cond.cuda(), n, seed=seed)
    eng = m._engine()

    def noise_at(step):
        z = torch.empty(n, D, device="cuda")
        L.check(L.lib().osd_op_randn(eng.handle, L.ptr(z), n, D, seed, 0, step, 0))
        return z.cpu()
    bufs = O.schedule_buffers("cosine", T)
    torch.set_num_threads(8)
    ref = O.sample(sd, bufs, cond, noise_at(T), noise_at, 3, 128)
    assert_close(out.cpu(), ref, CHAIN_RTOL, what="D=2000 T=1000 chain vs oracle")
    assert np.array_equal((out.cpu().numpy()[:, :50] > 0.5), (ref.numpy()[:, :50] > 0.5))


def test_sharding_chunking_graph_invariance():
    """Size-independent properties at the BASELINE shape: the sample of a row depends only on
    (seed, global row, its condition) -- not on chunking, streams, graph replay or how rows
    are sharded over ranks."""
    m, _ = full_model(3)
    T_small = config(FULL_H, T=25)
    m2 = BiologyAwareDiffusionModel(config=T_small, **FULL)
    m2.load_state_dict({k: v for k, v in m.state_dict().items() if k.startswith(("condition_embed", "unet"))}, strict=False)
    m2 = m2.cuda().eval()
    n = 5000
    cond = torch.randn(n, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    m2.sample_chunk_rows, m2.sample_streams, m2.use_graph = 32768, 1, False
    base = m2.sample(cond, n, seed=99)
    assert torch.isfinite(base).all()
    m2.sample_chunk_rows, m2.sample_streams, m2.use_graph = 1536, 3, True
    assert torch.equal(m2.sample(cond, n, seed=99), base)
    # two "ranks": rows [0,2600) and [2600,5000) with their global row offsets
    a = m2.sample(cond[:2600], 2600, seed=99, row_offset=0)
    b = m2.sample(cond[2600:], 2400, seed=99, row_offset=2600)
    assert torch.equal(torch.cat([a, b]), base)
    assert not torch.equal(m2.sample(cond, n, seed=100), base)


def test_errors_are_python_exceptions():
    m, _ = full_model(3)
    with pytest.raises(RuntimeError):
        m.sample(torch.zeros(3, 3, device="cuda"), 4)                # row mismatch
    with pytest.raises(RuntimeError):
        m.predict_noise(torch.zeros(2, 1999, device="cuda"), 5, torch.zeros(2, 3, device="cuda"))
    with pytest.raises(ValueError):
        m.p_sample(torch.zeros(2, 2000, device="cuda"), 1000, torch.zeros(2, 3, device="cuda"))
    with pytest.raises(RuntimeError):
        m.sample(torch.zeros(2, 3), 2)                               # CPU tensor, GPU model


@pytest.mark.parametrize("dims,hidden,cond_dim", [
    ((62, 5054, 26), [256, 512, 256], 3),      # the reference's real TARGET-OS shape: D = 5142, rows not 16-byte aligned
    ((5, 30, 3), [64, 128, 256, 64], 4),       # 4 hidden dims, cond_dim 4, D = 38 (D % 4 != 0), group widths 8/16/32
    ((10, 54, 0), [32], 2),                    # single hidden dim: bottleneck only, no encoder/decoder, no pathways
])
def test_odd_shapes_vs_oracle(dims, hidden, cond_dim):
    """Unaligned / odd extents take the guarded (non-FAST) kernel paths: chain, single step and
    training gradients against the oracle."""
    T = 12
    conf = config(hidden, T=T)
    shapes = O.param_shapes(*dims, cond_dim, hidden, 128)
    sd = O.init_state_dict(shapes, seed=21)
    gen = torch.Generator().manual_seed(5)
    for k in sd:
        if k.endswith((".1.weight", ".5.weight")) and sd[k].dim() == 1:
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=gen)
    m = BiologyAwareDiffusionModel(*dims, cond_dim, conf)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    D, n = sum(dims), 37
    cond = torch.randn(n, cond_dim, generator=gen)
    x_T = torch.randn(n, D, generator=gen)
    zs = torch.randn(T - 1, n, D, generator=gen)
    bufs = O.schedule_buffers("cosine", T)
    nh = len(hidden)
    ref = O.sample(sd, bufs, cond, x_T, lambda t: zs[T - 1 - t], nh, 128)
    out = m.sample(cond.cuda(), n, x_T=x_T.cuda(), noise=zs.cuda())
    assert_close(out.cpu(), ref, CHAIN_RTOL, what=f"chain {dims} {hidden}")
    # training gradients (eval mode: no dropout) through the autograd interface
    t = torch.randint(0, T, (n,), generator=gen)
    noise = torch.randn(n, D, generator=gen)
    x0 = torch.randn(n, D, generator=gen)
    ref_loss, ref_grads = O.training_loss_and_grads(sd, bufs, x0, cond, t, noise, nh, 128)
    loss = m(x0.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda())
    loss.backward()
    assert_close(loss.item(), ref_loss, 1e-5, what="loss")
    for k, p in m.named_parameters():
        assert_close(p.grad.cpu(), ref_grads[k], 5e-5, atol=1e-8, what=f"grad {k}")


@pytest.mark.parametrize("dims,hidden,n", [
    ((62, 5054, 26), [256, 512, 256], 300),     # the reference's real TARGET-OS dims (config.yaml / QUICKSTART.md:202): D = 5142 = 4 * 1285 + 2
    ((5, 30, 2), [256, 256], 129),              # D = 37 (one partial quad), one full row tile + 1 row
])
def test_unaligned_feature_dim_runs_on_the_padded_state(dims, hidden, n):
    """D % 4 != 0 with device-generated draws: both engines keep the chain state in an internal buffer whose rows are padded to
    a multiple of 4 floats (pad columns meet zero weights in input_proj and get eps = 0 from a packed output_proj), so the
    LDS-DMA / FAST tile code and the persistent chain kernel apply instead of the guarded scalar-load kernels.  Checked (i)
    against the oracle fed with the device's own Philox draws (osd_op_randn returns exactly what the kernels draw), chain
    tolerance 5e-5 * max|ref|, mask bit-equal away from the threshold; (ii) chain kernel vs per-layer kernels bit for bit.
    Reference: models/diffusion.py:427-449, utils/generate.py:135."""
    import ctypes as C
    from osteosarcoma_diffusionmodel_amd import _lib as L
    T, cond_dim = 10, 3
    D = sum(dims)
    assert D % 4 != 0
    conf = config(hidden, T=T)
    shapes = O.param_shapes(*dims, cond_dim, hidden, 128)
    sd = O.init_state_dict(shapes, seed=33)
    m = BiologyAwareDiffusionModel(*dims, cond_dim, conf)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    m.input_splitk = 0                          # engines are compared bit for bit below: single-pass input_proj (see test_gpu_chain.py)
    gen = torch.Generator().manual_seed(6)
    cond = torch.randn(n, cond_dim, generator=gen)
    seed, off = (7 << 34) + 99, 11
    eng = m._engine()

    def draws(step):
        a = torch.empty(n, D, device="cuda")
        L.check(L.lib().osd_op_randn(eng.handle, L.ptr(a), n, D, seed, off, step, 0))
        return a.cpu()

    x_T = draws(T)
    zs = {t: draws(t) for t in range(1, T)}
    bufs = O.schedule_buffers("cosine", T)
    ref = O.sample(sd, bufs, cond, x_T, lambda t: zs[t], len(hidden), 128)
    m.sampler = "graph"
    out, mask = m.sample(cond.cuda(), n, seed=seed, row_offset=off, return_mutation_mask=True)
    assert m.last_sampler == "graph"
    assert_close(out.cpu(), ref, CHAIN_RTOL, atol=1e-6, what=f"padded-state chain D={D}")
    md = dims[0]
    refm = (ref[:, :md] > 0.5).float()
    near = (ref[:, :md] - 0.5).abs() <= CHAIN_RTOL * ref.abs().max() + 1e-6
    assert ((mask.cpu() != refm) & ~near).sum().item() == 0
    assert torch.equal(mask, (out[:, :md] > 0.5).float())
    # eager launches (no hipGraph) and the persistent chain kernel: same bits
    m.use_graph = False
    out_e = m.sample(cond.cuda(), n, seed=seed, row_offset=off)
    assert torch.equal(out_e, out)
    m.sampler, m.chain_grid = "chain", 2
    out_c, mask_c = m.sample(cond.cuda(), n, seed=seed, row_offset=off, return_mutation_mask=True)
    assert m.last_sampler == "chain"
    assert torch.equal(out_c, out), f"max|d| = {(out_c - out).abs().max().item():.3e}"
    assert torch.equal(mask_c, mask)


def test_generate_scenarios_batches_the_scenarios_into_one_chain():
    """utils/generate.py:146-175 returns one dict per scenario; here the scenarios share ONE reverse chain (rows k*N .. (k+1)*N-1 =
    scenario k): the result must equal model.sample on the concatenated condition rows with the same seed, split by scenario,
    with the mutation mask the threshold of the same rows; ``batched=False`` keeps the reference's loop."""
    conf = config(SM_H, T=8)
    m = BiologyAwareDiffusionModel(config=conf, **SM).cuda().eval()
    gen = SyntheticPatientGenerator(m, conf, device="cuda")
    scen = [{"name": "a", "conditions": {"survival_time": 2000, "event_occurred": 0, "metastasis_at_diagnosis": 0}},
            {"name": "b", "conditions": {"survival_time": 300, "event_occurred": 1, "metastasis_at_diagnosis": 1}},
            {"name": "c", "conditions": {"survival_time": 800, "event_occurred": 0, "metastasis_at_diagnosis": 0}}]
    n = 37
    out = gen.generate_scenarios(scen, n, seed=99)
    assert list(out) == ["a", "b", "c"]
    cond = torch.cat([gen.create_conditions(n, s["conditions"]) for s in scen])
    ref = m.sample(cond, 3 * n, seed=99).cpu().numpy()
    for k, s in enumerate(scen):
        r = out[s["name"]]
        rows = slice(k * n, (k + 1) * n)
        assert r["mutations"].shape == (n, 8) and r["expression"].shape == (n, 24) and r["pathways"].shape == (n, 8)
        assert np.array_equal(r["expression"], ref[rows, 8:32]) and np.array_equal(r["pathways"], ref[rows, 32:])
        assert np.array_equal(r["mutations"], (ref[rows, :8] > 0.5).astype(float))
        assert np.array_equal(r["conditions"], cond[rows].cpu().numpy())
    loop = gen.generate_scenarios(scen, n, batched=False)
    assert list(loop) == ["a", "b", "c"] and all(loop[k]["expression"].shape == (n, 24) for k in loop)


def test_c_abi_error_codes():
    """The C ABI reports misuse through return codes + osd_last_error (never aborts): call order, bad
    arguments, unsupported architectures."""
    import ctypes as C
    from osteosarcoma_diffusionmodel_amd import _lib as L
    lib = L.lib()
    cfg = L.OsdConfig()
    cfg.mutation_dim, cfg.expression_dim, cfg.pathway_dim, cfg.condition_dim = 8, 24, 8, 3
    cfg.time_dim, cfg.n_hidden, cfg.num_steps, cfg.dropout_p, cfg.device = 128, 3, 10, 0.0, 0
    for i, v in enumerate((32, 64, 32)):
        cfg.hidden_dims[i] = v
    h = C.c_void_p()
    assert lib.osd_create(C.byref(cfg), C.byref(h)) == L.OSD_OK
    # every settable option reads back its default, and setting that default reads back the same value
    defaults = {"chunk_rows": 65536, "n_streams": 2, "sampler": 0, "train_squad": 2, "squad_panel": 0, "chain_variant": 0, "precision": 0,
                "chain_grid": 0, "input_splitk": 0, "cond_bwd_fused": 1, "chain_spin_budget": 500_000_000, "chain_wall_budget_ms": 0,
                "chain_steps_per_launch": 0, "chain_stagger": 30000, "train_streams": 2}
    v = C.c_int64()
    for name, default in defaults.items():
        assert lib.osd_get_option(h, name.encode(), C.byref(v)) == L.OSD_OK and v.value == default, name
        assert lib.osd_set_option(h, name.encode(), default) == L.OSD_OK, name
        v.value = -7
        assert lib.osd_get_option(h, name.encode(), C.byref(v)) == L.OSD_OK and v.value == default, name
    # retired A/B switches are unknown names to both calls
    for name in ("train_ksplit", "dual_dgrad", "train_input_splitk", "grouped_wgrad", "fused_gn_bwd", "wgrad_mid_flush"):
        assert lib.osd_set_option(h, name.encode(), 1) == L.OSD_EINVAL, name
        assert lib.osd_get_option(h, name.encode(), C.byref(v)) == L.OSD_EINVAL, name
    x = torch.zeros(4, 40, device="cuda")
    c = torch.zeros(4, 3, device="cuda")
    # weights before schedule, compute before weights
    arr = (C.c_void_p * 52)(*[x.data_ptr()] * 52)
    assert lib.osd_load_weights(h, arr, 52) == L.OSD_ESTATE and b"osd_set_schedule" in lib.osd_last_error()
    assert lib.osd_p_sample_step(h, L.ptr(x), 3, L.ptr(c), None, 4, 0, 0, L.ptr(x), 0) == L.OSD_ESTATE
    assert lib.osd_sample_chain(h, L.ptr(c), 4, None, None, 0, 0, L.ptr(x), None, 0) == L.OSD_ESTATE
    assert lib.osd_load_weights(h, arr, 51) == L.OSD_EINVAL
    assert lib.osd_set_option(h, b"chunk_rows", 0) == L.OSD_EINVAL and lib.osd_set_option(h, b"nope", 1) == L.OSD_EINVAL
    assert lib.osd_set_option(h, b"n_streams", 3) == L.OSD_OK
    assert lib.osd_destroy(h) == L.OSD_OK
    cfg.hidden_dims[1] = 24                          # divisible by 8 but group width 3: outside the fused kernels
    assert lib.osd_create(C.byref(cfg), C.byref(h)) == L.OSD_EUNSUPPORTED
    cfg.hidden_dims[1] = 20                          # not divisible by 8: GroupNorm(8, C) itself rejects it
    assert lib.osd_create(C.byref(cfg), C.byref(h)) == L.OSD_EINVAL
    cfg.hidden_dims[1] = 64
    cfg.device = 99
    assert lib.osd_create(C.byref(cfg), C.byref(h)) == L.OSD_EINVAL
    with pytest.raises(ValueError):                  # same conditions through the Python mirror
        BiologyAwareDiffusionModel(config=config([32, 24, 32]), **SM).cuda().sample(torch.zeros(1, 3, device="cuda"), 1)
    with pytest.raises(ValueError):
        BiologyAwareDiffusionModel(config=config([32, 20, 32]), **SM)


def test_million_patient_scale_and_row_addressing():
    """BASELINE config 5 scale (1 000 000 patients on one GPU; T shortened to keep the test in seconds): no index
    overflows with > 2^31 bytes per tensor, and any window of rows equals a separate small run at that row_offset
    (Philox draws are addressed by global row, so shards of any size reproduce the single-GPU population bitwise)."""
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(config=config(FULL_H, T=3), **FULL).cuda().eval()
    n = 1_000_000
    cond = torch.randn(n, 3, device="cuda")
    x, mask = m.sample(cond, n, seed=99, return_mutation_mask=True)
    assert x.shape == (n, 2000) and mask.shape == (n, 50)
    assert torch.isfinite(x).all().item()
    assert torch.equal(mask, (x[:, :50] > 0.5).float())
    for off, cnt in ((0, 257), (654_321, 1000), (n - 129, 129)):
        xs, ms = m.sample(cond[off:off + cnt].contiguous(), cnt, seed=99, row_offset=off, return_mutation_mask=True)
        assert torch.equal(xs, x[off:off + cnt]) and torch.equal(ms, mask[off:off + cnt])


def test_chain_with_trained_weights_vs_oracle(golden_dir):
    """parity with a briefly trained checkpoint -- the oracle trains the small model on CPU for 150
    AdamW steps on structured synthetic data, then the device runs the T = 200 reverse chain with the trained weights and
    the oracle's noise (the un-clamped x0_hat of the reference still amplifies the first steps: |x| reaches ~4e4, two
    orders below the random-weight chains); the mutation mask must match bit for bit away from the threshold."""
    T, rows, D = 200, 48, 40
    sd = {k: v.clone() for k, v in golden_small_sd(golden_dir).items() if k.startswith(("condition_embed", "unet"))}
    bufs = O.schedule_buffers("cosine", T)
    gen = torch.Generator().manual_seed(123)
    basis = torch.randn(4, D, generator=gen)
    def batch(n):
        x0 = torch.randn(n, 4, generator=gen) @ basis * 0.5 + 0.1 * torch.randn(n, D, generator=gen)
        x0[:, :8] = (x0[:, :8] > 0).float()
        return x0, torch.randn(n, 3, generator=gen)
    names = list(sd)
    m1 = [torch.zeros_like(sd[k]) for k in names]
    m2 = [torch.zeros_like(sd[k]) for k in names]
    first = last = None
    for step in range(1, 151):
        x0, c = batch(64)
        t = torch.randint(0, T, (64,), generator=gen)
        nz = torch.randn(64, D, generator=gen)
        loss, grads = O.training_loss_and_grads(sd, bufs, x0, c, t, nz, len(SM_H), 128)
        gl, _ = O.clip_grad_norm([grads[k] for k in names], 1.0)
        O.adamw_step([sd[k] for k in names], gl, m1, m2, step, lr=2e-3, weight_decay=1e-5)
        first = loss.item() if first is None else first
        last = loss.item()
    assert last < 0.9 * first                                    # it learned something
    cond = torch.randn(rows, 3, generator=gen)
    x_T = torch.randn(rows, D, generator=gen)
    zs = torch.randn(T - 1, rows, D, generator=gen)              # draw order t = T-1 .. 1
    ref = O.sample(sd, bufs, cond, x_T, lambda t: zs[T - 1 - t], len(SM_H), 128)
    m = BiologyAwareDiffusionModel(config=config(SM_H, T=T), **SM)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    out, mask = m.sample(cond.cuda(), rows, x_T=x_T.cuda(), noise=zs.cuda(), return_mutation_mask=True)
    assert_close(out, ref, CHAIN_RTOL, atol=1e-5, what="trained-weights chain")
    refm = (ref[:, :8] > 0.5).float()
    near = (ref[:, :8] - 0.5).abs() <= CHAIN_RTOL * ref.abs().max()
    assert ((mask.cpu() != refm) & ~near).sum().item() == 0
