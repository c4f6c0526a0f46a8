"""Validation loss on the device (the reference's `_step`, the number validation_step logs as valid_loss): the forward-diffusion and loss
kernels of csrc/sde.hip alone against torch, their generated-noise and per-row-key forms, the three models' `validation_loss` against the
REFERENCE's own `_step` (fixture F23, tools/make_golden_valid_loss.py) and the argument surface."""
import functools

import numpy as np
import pytest
import torch

from tests import valid_loss_cases as VC
from tests.backend import dev, setup_backend  # noqa: F401
from tests.test_convtasnet import TAG, TOL
from tests.test_row_seeds import ROW_SEEDS, _batch_invariant

# (B, F, T): one element; a row shorter than a block; one 64-frame bucket; more than 2048 * 256 elements per row - the grid-stride loop
# takes a second trip, with a ragged tail
SHAPES = [(1, 1, 1), (3, 3, 5), (2, 256, 64), (2, 263, 2001)]
KEY_SHAPES = [(3, 3, 5), (3, 256, 64)]                       # B = 3: a key per row
T_ROWS = torch.tensor([0.9, 0.5, 0.03])
# an fp64 sum rounded ONCE to fp32: 2^-24 = 6e-8 relative (the fp64 partial sums add 1e-16 each)
SUM_TOL = 2e-7
SEED, OFFSET = 2 ** 40 + 17, 3


def _sdes():
    from storm_amd.sdes import OUVESDE, OUVPSDE
    return {"ouve": OUVESDE(1.5, 0.05, 0.5, N=30), "ouvp": OUVPSDE(0.1, 2.0, 1, N=30)}


@functools.lru_cache(maxsize=None)
def _state(B, F, T):
    """(x0, y, z, score) complex64 [B,1,F,T] on the host, computed once per shape and left unchanged"""
    g = torch.Generator().manual_seed(100 * B + F + T)
    x0, y, z, score = (s * torch.randn(B, 1, F, T, dtype=torch.complex64, generator=g) for s in (0.3, 0.4, 1.0, 2.0))
    return x0, y, z, score


def _rho_rows(err, kind):
    """0.5 sum rho(err) per row: err as given (fp32), everything after it in fp64"""
    e = (err.to(torch.complex128) if err.is_complex() else err.double()).abs().flatten(1)
    return 0.5 * (e ** 2 if kind == "mse" else e).sum(1)


def _rel(got, want):
    return float(((got.double().cpu() - want) / want).abs().max())


# ---- 1. the perturbation kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,T", SHAPES)
@pytest.mark.parametrize("name", ["ouve", "ouvp"])
def test_perturb_kernel_is_the_reference_expression(dev, name, B, F, T):
    """mean + std.view(B,1,1,1) * z in fp32 on the CPU with the SDE's own `_mean` / `_std` (both operation orders of the mean), injected z:
    torch.equal - the operation order is the specification"""
    from storm_amd import ops
    sde = _sdes()[name]
    x0, y, z, _ = _state(B, F, T)
    t = T_ROWS[:B]
    want = sde._mean(x0, t, y) + sde._std(t).view(B, 1, 1, 1) * z
    got = ops.sde_perturb_rows(x0.to(dev), y.to(dev), sde.mean_factor_rows(t), sde._std(t), sde.MEAN_FORM, z=z.to(dev))
    assert got.dtype == torch.complex64 and torch.equal(got.cpu(), want)
    x_t, std = sde.marginal_prob_sample(x0.to(dev), t.to(dev), y.to(dev), z=z.to(dev))
    assert torch.equal(x_t.cpu(), want) and torch.equal(std.cpu(), sde._std(t)) and std.device == x_t.device


# ---- 2. generated noise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,T", KEY_SHAPES)
@pytest.mark.parametrize("name", ["ouve", "ouvp"])
def test_perturb_generated_noise(dev, name, B, F, T):
    """seed=, offset= draws what complex_randn(shape, seed, offset) holds; with row_seeds row b is the batch-1 call with seed = row_seeds[b]"""
    from storm_amd import ops
    sde = _sdes()[name]
    x0, y, _, _ = (v.to(dev) for v in _state(B, F, T))
    t = T_ROWS[:B]
    args = lambda sl: (x0[sl], y[sl], sde.mean_factor_rows(t[sl]), sde._std(t[sl]), sde.MEAN_FORM)
    z = ops.complex_randn(tuple(x0.shape), dev, SEED, OFFSET)
    drawn = ops.sde_perturb_rows(*args(slice(None)), seed=SEED, offset=OFFSET)
    assert torch.equal(drawn, ops.sde_perturb_rows(*args(slice(None)), z=z))
    rows = ops.sde_perturb_rows(*args(slice(None)), row_seeds=ROW_SEEDS[:B], offset=OFFSET)
    for b in range(B):
        assert torch.equal(rows[b:b + 1], ops.sde_perturb_rows(*args(slice(b, b + 1)), seed=ROW_SEEDS[b], offset=OFFSET)), b
    assert not torch.equal(rows[1], drawn[1])


# ---- 3. the loss kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,T", SHAPES)
@pytest.mark.parametrize("kind", ["mse", "mae"])
def test_dsm_loss_kernel(dev, kind, B, F, T):
    """0.5 sum rho(score std + z): the same err formed in fp32 by torch and summed in fp64, SUM_TOL; two runs equal bits; row b of the batch
    equals its batch-1 call bit for bit"""
    from storm_amd import ops
    _, _, z, score = _state(B, F, T)
    std = _sdes()["ouve"]._std(T_ROWS[:B])
    want = _rho_rows(score * std.view(B, 1, 1, 1) + z, kind)
    sd, zd, stdd = score.to(dev), z.to(dev), std.to(dev)
    got = ops.dsm_loss_rows(sd, stdd, z=zd, kind=kind)
    err = _rel(got, want)
    print(f"dsm_loss_rows {kind} {(B, F, T)}: worst row rel-L2 vs the fp64 sum {err:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (B,) and err < SUM_TOL
    assert torch.equal(got, ops.dsm_loss_rows(sd, stdd, z=zd, kind=kind))
    for b in range(B):
        assert torch.equal(got[b:b + 1], ops.dsm_loss_rows(sd[b:b + 1], stdd[b:b + 1], z=zd[b:b + 1], kind=kind)), b


@pytest.mark.parametrize("B,F,T", KEY_SHAPES)
@pytest.mark.parametrize("kind", ["mse", "mae"])
def test_dsm_loss_generated_noise_and_frames(dev, kind, B, F, T):
    """the re-drawn z (seed / row_seeds, the perturbation's key and offset) gives the injected-z bits; row_frames = [T, T - 1, 1] gives
    the loss of each row cropped to its frames (SUM_TOL: the blocking follows n) and changes the padded rows"""
    from storm_amd import ops
    _, _, _, score = _state(B, F, T)
    score = score.to(dev)
    std = _sdes()["ouvp"]._std(T_ROWS[:B]).to(dev)
    z = ops.complex_randn(tuple(score.shape), dev, SEED, OFFSET)
    inj = ops.dsm_loss_rows(score, std, z=z, kind=kind)
    assert torch.equal(ops.dsm_loss_rows(score, std, kind=kind, seed=SEED, offset=OFFSET), inj)
    zr = ops.complex_randn(tuple(score.shape), dev, 0, OFFSET, row_seeds=torch.tensor(ROW_SEEDS[:B]).to(dev))
    rows = ops.dsm_loss_rows(score, std, kind=kind, row_seeds=ROW_SEEDS[:B], offset=OFFSET)
    assert torch.equal(rows, ops.dsm_loss_rows(score, std, z=zr, kind=kind))
    for b in range(B):
        assert torch.equal(rows[b:b + 1], ops.dsm_loss_rows(score[b:b + 1], std[b:b + 1], kind=kind, seed=ROW_SEEDS[b], offset=OFFSET)), b
    frames = [T, T - 1, 1]
    got = ops.dsm_loss_rows(score, std, z=z, kind=kind, frames=frames)
    assert torch.equal(got[0], inj[0]) and not torch.equal(got[1], inj[1]) and not torch.equal(got[2], inj[2])
    for b, fr in enumerate(frames):
        crop = ops.dsm_loss_rows(score[b:b + 1, ..., :fr].contiguous(), std[b:b + 1], z=z[b:b + 1, ..., :fr].contiguous(), kind=kind)
        assert _rel(got[b:b + 1], crop.double().cpu()) < SUM_TOL, b
    with pytest.raises(ValueError):
        ops.dsm_loss_rows(score, std, z=z, kind=kind, frames=frames[:2])


# ---- 4. the pair losses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,T", SHAPES)
@pytest.mark.parametrize("kind", ["mse", "mae"])
@pytest.mark.parametrize("real", [False, True])
def test_pair_loss_kernel(dev, real, kind, B, F, T):
    """0.5 sum |a - b|^2 / 0.5 sum |a - b| of two spectrogram batches or two waveform batches: a - b in fp32 by torch, the sum in fp64"""
    from storm_amd import ops
    a, b, _, _ = _state(B, F, T)
    if real:
        a, b = torch.view_as_real(a).flatten(1)[:, :-1].contiguous(), torch.view_as_real(b).flatten(1)[:, :-1].contiguous()      # odd lengths
    want = _rho_rows(a - b, kind)
    ad, bd = a.to(dev), b.to(dev)
    got = ops.pair_loss_rows(ad, bd, kind=kind)
    err = _rel(got, want)
    print(f"pair_loss_rows {kind} real={real} {(B, F, T)}: worst row rel-L2 vs the fp64 sum {err:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (B,) and err < SUM_TOL
    assert torch.equal(got, ops.pair_loss_rows(ad, bd, kind=kind))
    for r in range(B):
        assert torch.equal(got[r:r + 1], ops.pair_loss_rows(ad[r:r + 1], bd[r:r + 1], kind=kind)), r
    if B == 3:
        frames = [T, T - 1, 1]
        if real:
            with pytest.raises(ValueError):
                ops.pair_loss_rows(ad, bd, kind=kind, frames=frames)
            return
        fr_rows = ops.pair_loss_rows(ad, bd, kind=kind, frames=frames)
        assert not torch.equal(fr_rows[1], got[1]) and not torch.equal(fr_rows[2], got[2])
        for r, fr in enumerate(frames):
            crop = _rho_rows((a - b)[r:r + 1, ..., :fr], kind)
            assert _rel(fr_rows[r:r + 1], crop) < SUM_TOL, r


@pytest.mark.parametrize("n,n_hat", [(1000, 1000), (4001, 4032), (4032, 4001)])
def test_sisdr_path_against_si_sdr_torch_in_fp64(dev, n, n_hat):
    """the `sisdr` loss is storm_si_sdr with eps = 1e-10 on the shorter length: si_sdr_torch (util/other.py:88-94) restated in fp64.  The
    sums run in fp64 and the dB value is rounded once to fp32: SUM_TOL of max(|dB|, 1)"""
    from storm_amd import ops
    g = torch.Generator().manual_seed(n)
    s = torch.randn(3, n, generator=g)
    sh = torch.zeros(3, n_hat)
    m = min(n, n_hat)
    sh[:, :m] = s[:, :m] * torch.tensor([[1.0], [0.5], [-2.0]]) + torch.tensor([[0.3], [1.0], [0.01]]) * torch.randn(3, m, generator=g)
    got = ops.si_sdr(s.to(dev), sh.to(dev), eps=1e-10).double().cpu()
    s64, h64 = s[:, :m].double(), sh[:, :m].double()
    alpha = (h64 * s64).sum(1, keepdim=True) / (s64 ** 2).sum(1, keepdim=True)
    want = 10 * torch.log10(1e-10 + ((alpha * s64) ** 2).sum(1) / (1e-10 + ((alpha * s64 - h64) ** 2).sum(1)))
    err = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
    print(f"si_sdr eps=1e-10 {(n, n_hat)}: {[round(float(v), 3) for v in want]} dB, rel-L2 of the worst row {err:.3e}")
    assert err < SUM_TOL


# ---- 5. the models against the reference's _step (F23) ----------------------------------------------------------------------------------
def _engine_classes():
    from storm_amd import model as M
    return {"score": M.ScoreModel, "disc": M.DiscriminativeModel, "storm": M.StochasticRegenerationModel}


def _case(name, golden, dev):
    """the case's engine model on `dev`, its inputs, and (t, z) of the reference's step - all regenerated from seeds and checked by hash"""
    g = golden["f23_valid_loss"]
    m, vals = VC.build(name, _engine_classes())
    x, y = VC.inputs(name)
    assert np.array_equal(VC.sha(vals), g[f"{name}_sha_weights"]) and np.array_equal(VC.sha([x, y]), g[f"{name}_sha_inputs"])
    kw = {}
    if name in VC.DRAWS:
        u, z = VC.draws(name)
        assert np.array_equal(VC.sha([u, z]), g[f"{name}_sha_draws"])
        kw = dict(t=torch.from_numpy(g[f"{name}_t"]), z=z)
    return m.to(dev), x, y, kw, g


# Every case runs in every precision on the GPU.  The simulator walks every lane of every kernel (20 s per NCSN++ evaluation of this batch):
# it runs one case of each model class, both SDEs and both loss kinds in fp32.
_SIM_CASES = ["score_ouvp_mse", "disc_ncsnpp_mae", "disc_convtasnet_sisdr", "storm_both_mse_mse"]
_MODEL_CASES = [pytest.param("hip", n, p, marks=pytest.mark.gpu) for n in VC.CASES for p in ("fp32", "bf16", "fp16")] + \
    [pytest.param("sim", n, "fp32") for n in _SIM_CASES]
_PREC = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.mark.parametrize("backend,name,prec", _MODEL_CASES)
def test_validation_loss_vs_reference(backend, name, prec, golden):
    """validation_loss with the reference's t and z against the reference's `_step` on the same weights and batch.  fp32: relative error of
    every returned loss < 1e-4 (the project's fp32 network bound); 16 bit: max(TOL, 2 x the reference's own error in that dtype, F23)."""
    dev = setup_backend(backend)
    m, x, y, kw, g = _case(name, golden, dev)
    m.set_precision(prec)
    dtype = _PREC[prec]
    got = m.validation_loss(x.to(dev), y.to(dev), **{k: v.to(dev) if k == "z" else v for k, v in kw.items()})
    got = got if isinstance(got, tuple) else (got,)
    want = g[f"{name}_loss"]
    assert len(got) == len(want)
    bound = TOL[dtype] if dtype == torch.float32 else max(TOL[dtype], 2 * float(g[f"{name}_referr_{TAG[dtype]}"]))
    errs = []
    for a, b in zip(got, want):
        assert (a is None) == bool(np.isnan(b))
        if a is not None:
            assert a.dtype == torch.float32 and a.dim() == 0
            errs.append(abs(float(a) - float(b)) / abs(float(b)))
    print(f"F23 {name} {prec}: " + " ".join(f"{e:.3e}" for e in errs) + f" rel-L2 of the loss vs the reference's _step (bound {bound:.1e})")
    assert max(errs) < bound, errs


# ---- 6. surface ---------------------------------------------------------------------------------------------------------------------------
def _analytic(sde):
    """a score of elementwise torch ops (no network: the simulator walks every lane)"""
    return lambda x, t, y, **kw: -(x - y) * (1 + 4 * y.abs()) / (sde._std(t.cpu()).to(x.device)[:, None, None, None] ** 2 + 0.1)


def _small_batch(dev):
    g = torch.Generator().manual_seed(77)
    x = 0.3 * torch.randn(3, 1, 8, 16, dtype=torch.complex64, generator=g)
    return x.to(dev), (x + 0.2 * torch.randn(3, 1, 8, 16, dtype=torch.complex64, generator=g)).to(dev)


def _score_model(dev, **kw):
    """ScoreModel around an analytic score (the constructor's network is not run)"""
    m = _engine_classes()["score"](**dict(VC.CASES["score_ouve_mse"][1], **kw))
    m._error_loading_ema = True
    m = m.eval().to(dev)
    m.forward = _analytic(m.sde)
    return m


def _storm_model(dev, **kw):
    m = _engine_classes()["storm"](**dict(VC.CASES["storm_both_mse_mse"][1], **kw))
    m._error_loading_ema = True
    m = m.eval().to(dev)
    m.forward_denoiser = lambda y, **k: 0.8 * y
    score = _analytic(m.sde)
    m.forward_score = lambda x, t, score_conditioning, sde_input, **k: score(x, t, sde_input)
    return m


def test_score_model_takes_the_mean_and_storm_the_sum_of_the_rows(dev):
    """ScoreModel._loss: torch.mean over the rows' 0.5 sums (model.py:113-122); StoRM's _reduce_op: 0.5 torch.sum over the whole batch
    (model.py:449, 468-481) - B = 3 separates the two.  The rows are the kernels' restated in torch (fp32 err, fp64 sums)."""
    x, y = _small_batch(dev)
    t = T_ROWS.clone()
    z = torch.randn(3, 1, 8, 16, dtype=torch.complex64, generator=torch.Generator().manual_seed(78)).to(dev)
    m = _score_model(dev)
    mean, std = m.sde.marginal_prob(x.cpu(), t, y.cpu())
    sig = std.view(3, 1, 1, 1)
    want = _rho_rows(m.forward(mean + sig * z.cpu(), t, y.cpu()) * sig + z.cpu(), "mse")
    rows = m.validation_loss(x, y, t=t, z=z, reduce=False)
    assert tuple(rows.shape) == (3,) and _rel(rows, want) < 1e-5
    loss = m.validation_loss(x, y, t=t, z=z)
    assert loss.dim() == 0 and torch.equal(loss, torch.mean(rows))
    s = _storm_model(dev, weighting_denoiser_to_score=0.25)
    yd = 0.8 * y.cpu()
    mean, std = s.sde.marginal_prob(x.cpu(), t, yd)
    want_s = _rho_rows(_analytic(s.sde)(mean + sig * z.cpu(), t, yd) * sig + z.cpu(), "mse")
    want_d = _rho_rows(yd - x.cpu(), "mse")
    l, ls, ld = s.validation_loss(x, y, t=t, z=z)
    assert abs(float(ls) / float(want_s.sum()) - 1) < 1e-5 and abs(float(ld) / float(want_d.sum()) - 1) < 1e-5
    assert abs(float(l) / (0.25 * float(ld) + 0.75 * float(ls)) - 1) < 1e-6
    rl, rs, rd = s.validation_loss(x, y, t=t, z=z, reduce=False)
    assert torch.equal(ls, rs.sum()) and torch.equal(ld, rd.sum()) and tuple(rl.shape) == (3,)
    s.loss_type_denoiser = "none"
    l, ls2, ld = s.validation_loss(x, y, t=t, z=z)
    assert ld is None and torch.equal(l, ls2) and torch.equal(ls2, ls)


def test_seeded_draws_and_frames(dev):
    """seed= fixes t and the noise; row_seeds= makes row b the batch-1 call with seed = row_seeds[b] (its t from its own generator);
    frames keeps the padding frames out; validation_epoch weights the micro-batches by their rows"""
    from storm_amd.util.inference import validation_epoch
    x, y = _small_batch(dev)
    m = _score_model(dev)
    a = m.validation_loss(x, y, seed=5, reduce=False)
    assert torch.equal(a, m.validation_loss(x, y, seed=5, reduce=False)) and not torch.equal(a, m.validation_loss(x, y, seed=6, reduce=False))
    rows = m.validation_loss(x, y, row_seeds=ROW_SEEDS, reduce=False)
    for b in range(3):
        assert torch.equal(rows[b:b + 1], m.validation_loss(x[b:b + 1], y[b:b + 1], seed=ROW_SEEDS[b], reduce=False)), b
    fr = m.validation_loss(x, y, row_seeds=ROW_SEEDS, frames=[16, 9, 1], reduce=False)
    assert torch.equal(fr[0], rows[0]) and float(fr[1]) < float(rows[1]) and float(fr[2]) < float(rows[2])
    ep = validation_epoch(m, [(x, y), (x[:1], y[:1], [9])], row_seeds=[ROW_SEEDS, ROW_SEEDS[1:2]])
    one = m.validation_loss(x[:1], y[:1], row_seeds=ROW_SEEDS[1:2], frames=[9])
    assert abs(ep - (3 * float(rows.mean()) + float(one)) / 4) < 1e-6 * abs(ep)
    s = _storm_model(dev)
    ep = validation_epoch(s, [(x, y), (x[:2], y[:2])], seed=3)
    assert len(ep) == 3 and abs(ep[0] - (0.5 * ep[2] + 0.5 * ep[1])) < 1e-5 * abs(ep[0])


def test_argument_errors(dev):
    x, y = _small_batch(dev)
    z = torch.zeros_like(x)
    for m in (_score_model(dev), _storm_model(dev)):
        for kw in (dict(seed=1, row_seeds=[1, 2, 3]), dict(seed=1, z=z), dict(z=z, row_seeds=[1, 2, 3]), dict(row_seeds=[1, 2])):
            with pytest.raises(ValueError):
                m.validation_loss(x, y, **kw)
    for kw in (dict(loss_type_denoiser="sisdr"), dict(loss_type_denoiser="mse_cplx+mag"), dict(loss_type_score="none"), dict(loss_type_score="sisdr")):
        with pytest.raises(NotImplementedError):                   # configure_losses (model.py:465-485)
            _storm_model(dev, **kw).validation_loss(x, y, seed=1)
    with pytest.raises(NotImplementedError):
        _score_model(dev, loss_type="sisdr").validation_loss(x, y, seed=1)


def test_convtasnet_mse_on_unequal_lengths_fails_as_upstream(dev):
    """a time-domain backbone returns its padded length: 'mse' against istft(x) of another length fails as upstream's subtraction does,
    naming both lengths ('sisdr' trims: F23)"""
    m, _ = VC.build("disc_convtasnet_sisdr", _engine_classes())
    m = m.to(dev)
    m.loss_type = "mse"
    g = torch.Generator().manual_seed(79)
    from storm_amd import ops
    x = 0.3 * torch.randn(1, 1, 256, 9, dtype=torch.complex64, generator=g).to(dev)        # 8 hops = 1024 samples
    padded = (ops.tasnet_frames(1024, m.dnn.win) - 1) * m.dnn.stride + m.dnn.win           # what the network returns (convtasnet.py:75-94)
    assert padded > 1024
    with pytest.raises(RuntimeError, match=rf"1024.*{padded}"):
        m.validation_loss(x, x)


_ROW_CASES = [pytest.param("hip", "score_ouve_mse", marks=pytest.mark.gpu), pytest.param("hip", "storm_both_mse_mse", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("backend,name", _ROW_CASES)
def test_rows_equal_their_batch1_calls_bf16(backend, name, golden):
    """validation_loss(row_seeds=) under storm_amd.set_batch_invariant(), bf16, the tiny networks of F23: row b of the batch equals its
    batch-1 call with seed = row_seeds[b] bit for bit - its t, its noise, its network rows and its sum do not see the batch"""
    dev = setup_backend(backend)
    m, x, y, _, _ = _case(name, golden, dev)
    m.set_precision("bf16")
    x, y = x.to(dev), y.to(dev)
    pick = (lambda out: out[0]) if name.startswith("storm") else (lambda out: out)
    with _batch_invariant(True):
        rows = pick(m.validation_loss(x, y, row_seeds=ROW_SEEDS, reduce=False))
        assert tuple(rows.shape) == (3,) and torch.isfinite(rows).all()
        for b in range(3):
            assert torch.equal(rows[b:b + 1], pick(m.validation_loss(x[b:b + 1], y[b:b + 1], seed=ROW_SEEDS[b], reduce=False))), b
