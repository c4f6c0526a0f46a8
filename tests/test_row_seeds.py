"""Per-utterance noise keys (row_seeds): a seeded result that does not depend on batching.

The one-seed noise path draws element i of row b from the Philox counter b * n + i, so a row's noise depends on its place in the
batch.  With a key per row (the storm_*_rs entry points) row b draws what the batch-1 call with seed = row_seeds[b] draws: these
tests hold every layer - kernels, samplers, models, the stream, the CLI - to "row b of the batched run == its own batch-1 run"."""
import os

import pytest
import torch

from oracle import ncsnpp_ref as NR
from tests.backend import dev, setup_backend  # noqa: F401
from tests.test_model import COMMON, score_model
from tests.util import rel_l2

ROW_SEEDS = [7, 2 ** 40 + 3, 2 ** 63 - 1]                   # both 32-bit key words in use, the largest key
SHAPES = [(3, 1000), (2, 256 * 5 + 7)]                      # no row length a multiple of the 256-thread block: a row ends inside a block
OFFSETS = [1, 5]
# fp32 rows against their batch-1 runs: the bound tests/test_model.py:710 (test_ragged_micro_batch_equals_per_utterance_runs) holds
# for injected noise - the draws are now the same numbers, so what is left is the same difference (kernel selection by batch size)
ROW_TOL = 1e-5


def _inputs(B, n, dev):
    g = torch.Generator().manual_seed(1000 + n)
    x, y, score = (torch.view_as_complex(0.3 * torch.randn(B, n, 2, generator=g)).to(dev) for _ in range(3))
    t = torch.tensor([0.9, 0.5, 0.2][:B]).to(dev)
    return dict(x=x, y=y, score=score, t=t)


def _kernel_cases():
    """name -> (fn(inputs, row slice, **keys) -> output tensors (the noisy state first, then x_mean), draws noise?)"""
    from storm_amd import ops
    from storm_amd.sdes import OUVESDE, OUVPSDE
    sde, psde = OUVESDE(1.5, 0.05, 0.5, N=30), OUVPSDE(0.1, 2.0, 1, N=30)
    cases = {
        "prior": (lambda i, sl, **k: (ops.ouve_prior(sde, i["y"][sl], **k),), True),
        "ald": (lambda i, sl, **k: ops.ouve_ald_step(sde, i["x"][sl].clone(), i["score"][sl], i["t"][sl], 0.5, **k), True),
        "sde_prior": (lambda i, sl, **k: (ops.sde_prior_rows(i["y"][sl], psde._std(i["t"][sl]), **k),), True),
    }
    for kind in (0, 1):
        for nf in (0, 1):
            cases[f"predictor_k{kind}_nf{nf}"] = (lambda i, sl, kind=kind, nf=nf, **k: ops.ouve_predictor_step(
                sde, i["x"][sl].clone(), i["score"][sl], i["y"][sl], i["t"][sl], kind=kind, noise_free=bool(nf), **k), not nf)
            cases[f"sde_predictor_k{kind}_nf{nf}"] = (lambda i, sl, kind=kind, nf=nf, **k: ops.sde_predictor_step_rows(
                psde, i["x"][sl].clone(), i["score"][sl], i["y"][sl], i["t"][sl], kind=kind, noise_free=bool(nf), **k), not nf)
    return cases


KERNEL_CASES = ["prior", "ald", "sde_prior"] + [f"{p}_k{k}_nf{nf}" for p in ("predictor", "sde_predictor") for k in (0, 1) for nf in (0, 1)]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("B,n", SHAPES)
def test_complex_randn_rows(dev, B, n, offset):
    """row b of the rows form == storm_complex_randn(n, row_seeds[b], offset), bit for bit"""
    from storm_amd import ops
    keys = torch.tensor(ROW_SEEDS[:B], dtype=torch.int64).to(dev)
    z = ops.complex_randn((B, n), dev, 0, offset, row_seeds=keys)
    for b in range(B):
        assert torch.equal(z[b], ops.complex_randn((n,), dev, ROW_SEEDS[b], offset)), b
    assert not torch.equal(z[0], z[1]) and torch.isfinite(torch.view_as_real(z)).all()
    assert abs(float(z.abs().pow(2).mean()) - 1.0) < 0.1                   # a standard complex normal: E |z|^2 = 1


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("B,n", SHAPES)
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernel_rows_equal_their_batch1_calls(dev, name, B, n, offset):
    """Every noise-drawing entry point, both predictor kinds, with and without the noise term: row b of the row_seeds call is BIT-equal
    (x and x_mean) to the existing entry point called on that row alone with seed = row_seeds[b]; and the table is really read - with
    every key equal to s the result equals today's batched seed = s call in row 0 and differs from it in every later row (a
    noise-free predictor step draws nothing: there the two are equal everywhere)."""
    fn, draws = _kernel_cases()[name]
    ins = _inputs(B, n, dev)
    keys = torch.tensor(ROW_SEEDS[:B], dtype=torch.int64).to(dev)
    batched = fn(ins, slice(None), offset=offset, row_seeds=keys)
    for b in range(B):
        alone = fn(ins, slice(b, b + 1), seed=ROW_SEEDS[b], offset=offset)
        assert len(alone) == len(batched)
        for got, want in zip(batched, alone):
            assert torch.equal(got[b:b + 1], want), (name, b)
    s = ROW_SEEDS[1]
    same_key = fn(ins, slice(None), offset=offset, row_seeds=torch.full((B,), s, dtype=torch.int64).to(dev))[0]
    one_seed = fn(ins, slice(None), seed=s, offset=offset)[0]
    assert torch.equal(same_key[0], one_seed[0])
    for b in range(1, B):
        assert torch.equal(same_key[b], one_seed[b]) == (not draws), (name, b)
    if draws:                        # rows with one key and one counter range draw the same numbers: x - x_mean is row-independent up to its scale
        assert not torch.equal(batched[0][0], batched[0][1])


def test_row_longer_than_the_grid_takes_the_stride_loop(dev):
    """The row launch caps at 2048 blocks of 256 threads: a row of 2048 * 256 + 7 elements sends the first 7 threads round the
    grid-stride loop a second time (no other case has a row that long).  The updates are elementwise and the noise is injected,
    so nothing depends on an element's position: the call on the whole row is BIT-equal to the same call on the first
    2048 * 256 elements and on the 7-element tail."""
    from storm_amd import ops
    from storm_amd.sdes import OUVESDE, OUVPSDE
    sde, psde = OUVESDE(1.5, 0.05, 0.5, N=30), OUVPSDE(0.1, 2.0, 1, N=30)
    head = 2048 * 256
    ins = _inputs(1, head + 7, dev)
    ins["z"] = torch.view_as_complex(torch.randn(1, head + 7, 2, generator=torch.Generator().manual_seed(5))).to(dev)
    t = ins["t"]
    calls = {
        "ouve_prior": lambda i: (ops.ouve_prior(sde, i["y"], z=i["z"]),),
        "ouve_predictor_step": lambda i: ops.ouve_predictor_step(sde, i["x"].clone(), i["score"], i["y"], t, kind=0, z=i["z"]),
        "sde_predictor_step_rows": lambda i: ops.sde_predictor_step_rows(psde, i["x"].clone(), i["score"], i["y"], t, kind=0, z=i["z"]),
        "sde_pf_drift_rows": lambda i: (ops.sde_pf_drift_rows(i["x"], i["y"], i["score"], psde.drift_rows(t), psde.diffusion(t)),),
    }
    parts = [{k: v[:, sl].contiguous() for k, v in ins.items() if k != "t"} for sl in (slice(None, head), slice(head, None))]
    for name, fn in calls.items():
        whole, first, tail = fn(ins), fn(parts[0]), fn(parts[1])
        for w, a, b in zip(whole, first, tail):
            assert w.shape == (1, head + 7) and torch.equal(w, torch.cat([a, b], 1)), name


# ---------------------------------------------------------------- samplers and models (tiny nets, F = 256, one 64-frame bucket, N = 3)
def _ouvp_model(dev):
    from storm_amd.data_module import SpecsDataModule
    from storm_amd.model import ScoreModel
    m = ScoreModel(backbone="ncsnpp", sde="ouvp", data_module_cls=SpecsDataModule, beta_min=0.1, beta_max=2.0, stiffness=1,
                   spec_factor=0.15, spec_abs_exponent=0.5, nf=8)
    m.dnn.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=81))
    m._error_loading_ema = True
    return m.eval().to(dev)


def _storm_model(dev):
    from storm_amd.model import StochasticRegenerationModel
    m = StochasticRegenerationModel(backbone_denoiser="ncsnpp", backbone_score="ncsnpp", condition="both", **dict(COMMON))
    m.denoiser_net.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=2, discriminative=True), seed=42))
    m.score_net.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=6), seed=43))
    m._error_loading_ema = True
    return m.eval().to(dev)


class _batch_invariant:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import storm_amd
        if self.on:
            storm_amd.set_batch_invariant(True)

    def __exit__(self, *exc):
        import storm_amd
        if self.on:
            storm_amd.set_batch_invariant(False)


COMBOS = {"reverse_diffusion+ald": ("ouve", "reverse_diffusion", "ald"), "euler_maruyama+langevin": ("ouve", "euler_maruyama", "langevin"),
          "ouvp+none": ("ouvp", "reverse_diffusion", "none")}


def _analytic_score(sde):
    """A score made of elementwise torch ops only (its strength follows |y| element by element, so the rows differ).  No reduction:
    torch plans a row mean by the batch size, and the last bit of a row's mean - then of its whole score - would follow the batch."""
    return lambda x, t, y, **kw: -(x - y) * (1 + 4 * y.abs()) / (sde._std(t)[:, None, None, None] ** 2 + 0.1)


@pytest.mark.parametrize("combo", list(COMBOS))
def test_pc_sampler_rows_equal_their_batch1_runs_analytic_score(dev, combo):
    """get_pc_sampler(row_seeds=) with a per-row analytic score on both backends (no network: the simulator walks every lane), 3 rows of
    256 x 64, N = 3: every predictor / corrector family of both SDEs (the Langevin corrector draws its z through the rows form).
    The score's torch ops and every kernel are per row, so row b is BIT-equal to the batch-1 run with seed = row_seeds[b]."""
    from storm_amd.sampling import get_pc_sampler
    from storm_amd.sdes import OUVESDE, OUVPSDE
    kind, pred, corr = COMBOS[combo]
    sde = OUVESDE(1.5, 0.05, 0.5, N=3) if kind == "ouve" else OUVPSDE(0.1, 2.0, 1, N=3)
    Y = torch.view_as_complex(0.3 * torch.randn(3, 1, 256, 64, 2, generator=torch.Generator().manual_seed(8))).to(dev)
    kw = dict(sde=sde, score_fn=_analytic_score(sde), eps=0.03, snr=0.5, langevin_per_row=True)
    x, nfe = get_pc_sampler(pred, corr, y=Y, row_seeds=ROW_SEEDS, **kw)()
    assert nfe == 3 * (1 + (corr != "none")) and torch.isfinite(torch.view_as_real(x)).all()
    for b in range(3):
        xb, _ = get_pc_sampler(pred, corr, y=Y[b:b + 1], seed=ROW_SEEDS[b], **kw)()
        assert torch.equal(x[b], xb[0]), (combo, b)
    x1, _ = get_pc_sampler(pred, corr, y=Y, seed=ROW_SEEDS[0], **kw)()          # the one-seed stream: row 0 the same draws, later rows not
    assert torch.equal(x1[0], x[0]) and not torch.equal(x1[1], x[1])


def test_ode_sampler_rows_equal_their_batch1_runs_analytic_score(dev):
    """get_ode_sampler(row_seeds=, per_row=True): the keys serve the prior draw, made on the whole batch before any row leaves it - every
    row's end state and evaluation count are those of its batch-1 run with seed = row_seeds[b] (rows of different stiffness: different
    step sequences, the early finishers leave the batch)"""
    from storm_amd.sampling import get_ode_sampler
    from storm_amd.sdes import OUVESDE
    sde = OUVESDE(1.5, 0.05, 0.5, N=30)
    g = torch.Generator().manual_seed(12)
    Y = (torch.view_as_complex(torch.randn(3, 1, 8, 16, 2, generator=g)) * torch.tensor([0.1, 0.4, 1.5])[:, None, None, None]).to(dev)
    sampler = get_ode_sampler(sde, _analytic_score(sde), y=Y, eps=0.03, per_row=True, row_seeds=ROW_SEEDS)
    x, nfe = sampler()
    assert nfe == max(sampler.nfev_rows) and len(set(sampler.nfev_rows)) > 1
    for b in range(3):
        alone = get_ode_sampler(sde, _analytic_score(sde), y=Y[b:b + 1], eps=0.03, per_row=True, seed=ROW_SEEDS[b])
        xb, nb = alone()
        assert nb == sampler.nfev_rows[b] and torch.equal(xb, x[b:b + 1]), b


# The tiny-network cases below are what the issue of this feature sets (F = 256, one 64-frame bucket, N = 3, every row against its
# batch-1 run) and run in full on the GPU.  The simulator walks every lane of every kernel (8 s per row and network evaluation): it
# runs the kernels, the samplers with an analytic score (above) and ONE network case with one reverse step and the last row compared.
_PC_NET_CASES = [pytest.param("hip", c, p, marks=pytest.mark.gpu) for c in COMBOS for p in ("fp32", "bf16", "fp16")] + \
    [pytest.param("sim", "ouvp+none", "fp32")]


@pytest.mark.parametrize("backend,combo,prec", _PC_NET_CASES)
def test_pc_sampler_rows_equal_their_batch1_runs(backend, combo, prec):
    """get_pc_sampler(row_seeds=) around the tiny NCSN++ on a 3-row batch.  fp32: row b equals the batch-1 run with seed = row_seeds[b]
    to ROW_TOL; bf16 / fp16 under set_batch_invariant: bit for bit."""
    dev = setup_backend(backend)
    sde, pred, corr = COMBOS[combo]
    m = score_model(dev) if sde == "ouve" else _ouvp_model(dev)
    m.set_precision(prec)
    Y = torch.view_as_complex(0.3 * torch.randn(3, 1, 256, 64, 2, generator=torch.Generator().manual_seed(8))).to(dev)
    N = 3 if backend == "hip" else 1
    kw = dict(N=N, snr=0.5, corrector_steps=1, langevin_per_row=True)
    with _batch_invariant(prec != "fp32"):
        x, nfe = m.get_pc_sampler(pred, corr, Y, row_seeds=ROW_SEEDS, **kw)()
        assert nfe == N * (1 + (corr != "none")) and torch.isfinite(torch.view_as_real(x)).all()
        worst = 0.0
        for b in (range(3) if backend == "hip" else (2,)):
            xb, _ = m.get_pc_sampler(pred, corr, Y[b:b + 1], seed=ROW_SEEDS[b], **kw)()
            if prec == "fp32":
                worst = max(worst, rel_l2(x[b].cpu(), xb[0].cpu()))
            else:
                assert torch.equal(x[b], xb[0]), (combo, prec, b)
        if prec == "fp32":
            print(f"row_seeds {combo} fp32: worst row rel-L2 vs its batch-1 seeded run {worst:.2e}")
            assert worst < ROW_TOL


@pytest.fixture
def gpu():
    return setup_backend("hip")


def _ragged(rows, dev):
    y = torch.zeros(len(rows), max(w.numel() for w in rows))
    for k, w in enumerate(rows):
        y[k, :w.numel()] = w
    return y.to(dev), [w.numel() for w in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["score", "storm"])
def test_enhance_batch_utterance_does_not_see_its_companions(gpu, kind):
    """ScoreModel / StochasticRegenerationModel.enhance_batch(row_seeds=), batch-invariant bf16, ragged 3-row micro-batches of one
    64-frame bucket: the same utterance with the same key at row 0 of one batch and at row 2 of another batch, with other
    companions of other lengths, comes out bit-equal."""
    dev = gpu
    m = score_model(dev) if kind == "score" else _storm_model(dev)
    m.set_precision("bf16")
    g = torch.Generator().manual_seed(15)
    u, a1, a2, b0, b1 = (0.1 * torch.randn(n, generator=g) for n in (4500, 5003, 4225, 4100, 4800))
    kw = dict(N=3, snr=0.5)
    with _batch_invariant(True):
        ya, la = _ragged([u, a1, a2], dev)
        yb, lb = _ragged([b0, b1, u], dev)
        xa = m.enhance_batch(ya, lengths=la, row_seeds=[11, 12, 13], **kw)
        xb = m.enhance_batch(yb, lengths=lb, row_seeds=[2 ** 50 + 1, 14, 11], **kw)
    assert torch.isfinite(xa).all() and float(xa[0, :4500].abs().max()) > 0
    assert torch.equal(xa[0, :4500], xb[2, :4500])
    assert not torch.equal(xa[1, :4100], xb[0, :4100])


@pytest.mark.gpu
def test_ode_rows_equal_their_batch1_runs(gpu):
    """ODE sampler, fp32, one step controller per row: row_seeds keys the prior draw, which is made before rows leave the batch - every
    row's wav (ROW_TOL) and its evaluation count (exactly) equal its batch-1 run with seed = row_seeds[b]"""
    dev = gpu
    m = score_model(dev)
    g = torch.Generator().manual_seed(16)
    rows = [0.1 * torch.randn(n, generator=g) for n in (4500, 5003, 4225)]
    y, lens = _ragged(rows, dev)
    kw = dict(sampler_type="ode", N=3, per_row=True, rtol=2e-3, atol=2e-3)
    x, nfe = m.enhance_batch(y, lengths=lens, row_seeds=ROW_SEEDS, return_nfe=True, **kw)
    nfev_rows = list(m.last_nfev_rows)
    assert nfe == max(nfev_rows)
    for b in range(3):
        xb, nb = m.enhance_batch(rows[b][None].to(dev), seed=ROW_SEEDS[b], return_nfe=True, **kw)
        e = rel_l2(x[b, :lens[b]].cpu(), xb[0].cpu())
        print(f"row_seeds ode row {b}: nfev {nfev_rows[b]} (batch-1: {nb}), wav rel-L2 vs its batch-1 seeded run {e:.2e}")
        assert nb == nfev_rows[b] and m.last_nfev_rows == [nb]
        assert e < ROW_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("grouped", [True, False])
def test_enhance_stream_row_seeds(gpu, grouped):
    """enhance_stream(row_seeds=) on three micro-batches of three frame buckets == the micro-batches' own enhance_batch calls with the
    same keys, bit for bit (a nf = 8 network has no layer with a grouped kernel), in lockstep around grouped network calls and one
    after the other"""
    dev = gpu
    m = score_model(dev)
    g = torch.Generator().manual_seed(31)
    lens = [[5003, 4500], [9000], [16100, 15000, 14100]]              # 64-, 128- and 192-frame buckets
    batches, keys = [], []
    for p, bl in enumerate(lens):
        y, _ = _ragged([0.1 * torch.randn(n, generator=g) for n in bl], dev)
        batches.append((y, bl if len(set(bl)) > 1 else None))
        keys.append([2 ** 33 * p + k + 1 for k in range(len(bl))])
    kw = dict(N=3, corrector="ald", snr=0.5)
    own = [m.enhance_batch(yb, lengths=bl, row_seeds=ks, **kw) for (yb, bl), ks in zip(batches, keys)]
    outs = m.enhance_stream(batches, grouped=grouped, row_seeds=keys, **kw)
    assert (m.last_group_calls is not None) == grouped
    for p in range(len(lens)):
        assert torch.equal(outs[p], own[p]), p


def test_row_seeds_argument_errors(dev):
    from storm_amd import ops
    from storm_amd.sampling import NoiseSource, get_ode_sampler, get_pc_sampler
    from storm_amd.sdes import OUVESDE
    m = score_model(dev)
    y = torch.zeros(2, 4500).to(dev)
    with pytest.raises(ValueError):
        m.enhance_batch(y, row_seeds=[1, 2], seed=3)
    with pytest.raises(ValueError):
        m.enhance_batch(y, row_seeds=[1, 2, 3])                      # three keys, two rows
    with pytest.raises(ValueError):
        m.enhance_batch(y, row_seeds=[1, 2 ** 63])                   # outside [0, 2^63)
    with pytest.raises(ValueError):
        m.enhance_batch(y, sampler_type="ode", row_seeds=[1])
    with pytest.raises(ValueError):
        m.enhance_stream([(y, None)], row_seeds=[[1, 2]], seed=3)
    with pytest.raises(ValueError):
        m.enhance_stream([(y, None)], row_seeds=[[1, 2]], seeds=[3])
    with pytest.raises(ValueError):
        m.enhance_stream([(y, None)], row_seeds=[[1, 2], [3]])       # two key lists, one micro-batch
    with pytest.raises(ValueError):
        NoiseSource(row_seeds=[1], noise_fn=lambda: None)
    sde = OUVESDE(1.5, 0.05, 0.5, N=3)
    Y = torch.zeros(2, 1, 8, 16, dtype=torch.complex64).to(dev)
    with pytest.raises(ValueError):
        get_pc_sampler("reverse_diffusion", "ald", sde=sde, score_fn=None, y=Y, row_seeds=[1, 2], seed=0)
    with pytest.raises(ValueError):
        get_ode_sampler(sde, None, y=Y, row_seeds=[1, 2], seed=0)
    with pytest.raises(ValueError):
        ops.ouve_prior(sde, Y, row_seeds=torch.tensor([1, 2, 3]).to(dev))
    with pytest.raises(ValueError):
        ops.ouve_prior(sde, Y, row_seeds=torch.tensor([1.0, 2.0]).to(dev))


def test_utterance_key_is_a_function_of_seed_and_name():
    import hashlib
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("enhancement_cli", os.path.join(root, "enhancement.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    h = int.from_bytes(hashlib.sha256(b"u0.wav").digest()[:8], "little")
    assert cli.utterance_key(3, "/some/dir/u0.wav") == cli.utterance_key(3, "u0.wav") == (3 + h) % 2 ** 63
    assert cli.utterance_key(3, "u0.wav") != cli.utterance_key(3, "u1.wav") != cli.utterance_key(4, "u1.wav")
    assert 0 <= cli.utterance_key(2 ** 63 - 1, "u0.wav") < 2 ** 63


@pytest.mark.gpu
def test_enhancement_cli_utterance_seed(tmp_path):
    """enhancement.py --utterance-seed: a file's wav depends on (seed, its name, its samples, precision) only.  Four files of two
    lengths enhanced together (--batch 4 --group 2: two 2-row micro-batches in lockstep) and two of them alone in another directory
    (--batch 1: one file per call), batch-invariant bf16: the shared files are byte-equal.  (With --seed 3 the two layouts seed
    their buckets by the first file's index in the directory, so they need not agree - not asserted.)"""
    import subprocess
    import sys

    import numpy as np
    from scipy.io import wavfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sd = NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=5)
    ckpt = os.path.join(tmp_path, "m.ckpt")
    torch.save({"state_dict": {"dnn." + k: v for k, v in sd.items()}, "hyper_parameters": dict(backbone="ncsnpp", **COMMON)}, ckpt)
    g = torch.Generator().manual_seed(9)
    files = {"a0.wav": 6000, "a1.wav": 6000, "b0.wav": 9100, "b1.wav": 9100}
    all4, two = os.path.join(tmp_path, "all4"), os.path.join(tmp_path, "two")
    os.makedirs(all4)
    os.makedirs(two)
    for name, n in files.items():
        w = (0.1 * torch.randn(n, generator=g)).numpy().astype(np.float32)
        wavfile.write(os.path.join(all4, name), 16000, w)
        if name in ("a1.wav", "b0.wav"):
            wavfile.write(os.path.join(two, name), 16000, w)
    env = {k: v for k, v in dict(os.environ, PYTHONPATH=root).items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = ["--ckpt", ckpt, "--mode", "score-only", "--N", "3", "--corrector", "ald", "--utterance-seed", "3", "--batch-invariant", "--precision", "bf16"]
    outs = []
    for src, extra in ((all4, ["--batch", "4", "--group", "2"]), (two, ["--batch", "1"])):
        out = src + "_enhanced"
        r = subprocess.run([sys.executable, os.path.join(root, "enhancement.py"), "--test_dir", src, "--enhanced_dir", out] + common + extra,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(out)
    for name in ("a1.wav", "b0.wav"):
        a, b = (open(os.path.join(o, name), "rb").read() for o in outs)
        sr, x = wavfile.read(os.path.join(outs[0], name))
        assert x.shape == (files[name],) and np.isfinite(x).all() and float(np.abs(x).max()) > 0
        assert a == b, name
    r = subprocess.run([sys.executable, os.path.join(root, "enhancement.py"), "--test_dir", two, "--enhanced_dir", outs[1]] + common + ["--seed", "3"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "exclude" in (r.stderr + r.stdout)
