"""The host simulator's wave schedules (STORM_SIM_WAVES, tests/sim/hip_host_shim.h): which wave of a workgroup gets ahead of
which.  Three things are pinned here, none of them on a GPU:

1. the hazard zoo (tests/sim/hazard_zoo.cpp): toy kernels with a correct and a BROKEN twin.  Every correct twin is exact under
   every schedule x DMA mode; every broken twin is wrong under exactly the schedules of BROKEN_UNDER - and most of them pass
   under the default schedule, which is the gap the schedules close;
2. the real kernels: per schedule one inner pytest run over SELECTION, the smallest existing cases that reach every kernel file
   that declares LDS (at least two waves per workgroup; "@8" / STORM_CONV_CUS=8 cases walk several tiles per workgroup);
3. COVERAGE names every such kernel file, so a new one fails here until it is given a case.

The schedule is fixed per loaded simulator library, so everything that depends on it runs in a subprocess."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.sim import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES = ["", "reverse", "first", "last"]                   # "" = unset: the ascending sweep
SEEDS = ["seed:1", "seed:7"]
DMAS = ["", "late"]                                        # "" = unset: a copy lands at once


def _env(waves, dma):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k, v in (("STORM_SIM_WAVES", waves), ("STORM_SIM_DMA", dma)):
        env.pop(k, None)
        if v:
            env[k] = v
    return env


def _run_zoo(waves, dma):
    r = subprocess.run([sys.executable, "-m", "tests.sim.zoo"], cwd=ROOT, env=_env(waves, dma), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


_zoo = functools.lru_cache(maxsize=None)(_run_zoo)


# ---- what the zoo's kernels compute, restated in numpy ------------------------------------------------------------------------
def _expected(kernel):
    src = zoo.source(kernel).astype(np.uint64)
    if kernel.startswith("raw"):
        return [int(v) for v in src[0][::-1]]                                  # consumer lane l reads word 63 - l
    tid = np.arange(128)
    acc = np.zeros(128, dtype=np.uint64)
    for t in range(src.shape[0]):
        if kernel == "war_ring":
            acc = (acc * 31 + src[t][(tid + 64) & 127] + src[t][tid]) & 0xffffffff
        else:                                                                  # the other wave's 16 bytes, word by word
            for e in range(4):
                acc = (acc * 31 + src[t][((tid + 64) & 127) * 4 + e]) & 0xffffffff
    return [int(v) for v in acc]


# The table: (STORM_SIM_WAVES, STORM_SIM_DMA) under which each BROKEN twin computes something else than its correct twin.
#   raw_below       wave 0 writes, wave 1 reads at once, no barrier         : whenever wave 1 moves first
#   raw_below_busy  the same, the reader two yield points into its phase    : only a whole phase of skew (the sweeps let wave 0 through)
#   raw_above_busy  wave 1 writes, wave 0 reads two yield points later      : only when wave 0 runs a whole phase ahead
#   war_ring        ring slot refilled one barrier early                    : only a whole phase of skew, either way round
#   dma_war         the same refill by LDS-DMA                              : a whole phase of skew AND a copy that lands at once
#   dma_raw         fragment read before the counted wait                   : a copy that lands late, under any wave order
BROKEN_UNDER = {
    "raw_below": {("reverse", ""), ("reverse", "late"), ("last", ""), ("last", "late")},
    "raw_below_busy": {("last", ""), ("last", "late")},
    "raw_above_busy": {("first", ""), ("first", "late")},
    "war_ring": {("first", ""), ("first", "late"), ("last", ""), ("last", "late")},
    "dma_war": {("first", ""), ("last", "")},
    "dma_raw": {(w, "late") for w in WAVES},
}


def test_table_names_every_zoo_kernel():
    assert set(BROKEN_UNDER) == set(zoo.KERNELS)
    assert all(BROKEN_UNDER.values()), "a broken twin that no schedule catches: the schedule set is incomplete"


@pytest.mark.parametrize("dma", DMAS, ids=["atonce", "late"])
@pytest.mark.parametrize("waves", WAVES + SEEDS, ids=lambda w: w.replace(":", "") or "unset")
def test_correct_twins_are_exact_under_every_schedule(waves, dma):
    got = _zoo(waves, dma)
    for kernel in zoo.KERNELS:
        assert got[kernel]["correct"] == _expected(kernel), (kernel, waves, dma)


@pytest.mark.parametrize("kernel", list(BROKEN_UNDER))
def test_broken_twin_is_wrong_under_its_listed_schedules_only(kernel):
    want = _expected(kernel)
    wrong = {(w, d) for w in WAVES for d in DMAS if _zoo(w, d)[kernel]["broken"] != want}
    assert wrong == BROKEN_UNDER[kernel]


def test_default_schedule_alone_misses_broken_twins():
    """The gap, as an assertion: with STORM_SIM_WAVES unset every wave-order mistake of the zoo passes (only the late-DMA
    bracket catches anything, and only the fragment-before-wait twin)."""
    missed = [k for k in zoo.KERNELS if _zoo("", "")[k]["broken"] == _expected(k) and _zoo("", "late")[k]["broken"] == _expected(k)]
    assert missed == ["raw_below", "raw_below_busy", "raw_above_busy", "war_ring", "dma_war"]


def test_seeded_schedule_replays_from_its_seed():
    a, b = _run_zoo("seed:7", ""), _run_zoo("seed:7", "")
    assert a == b                                             # broken twins included: a failure is reproducible
    assert _zoo("seed:1", "")["raw_below"]["broken"] != _expected("raw_below")       # and a seeded order does find a race


def test_unknown_schedule_is_refused():
    r = subprocess.run([sys.executable, "-m", "tests.sim.zoo"], cwd=ROOT, env=_env("sideways", ""), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "STORM_SIM_WAVES=sideways" in r.stderr


# ---- the real kernels under the skewed schedules ---------------------------------------------------------------------------------
OPS, NET = "tests/test_ops.py::", "tests/test_net.py::"
# kernel file -> the cases that run it under every skewed schedule (every workgroup of these has at least two waves)
COVERAGE = {
    "conv_igemm.hip": [OPS + "test_conv_pipelined_kernels[sim-gn_fused@8-7]", OPS + "test_conv_persistent_tile_loop[sim-3-dtype1]",
                       OPS + "test_conv_persistent_tile_loop[sim-1-dtype0]", OPS + "test_conv_fused_groupnorm_apply[sim-dtype1]"],
    "conv_pipe.hip": [OPS + "test_conv_pipelined_kernels[sim-gn_fused@8-3]", OPS + "test_conv_pipelined_kernels[sim-deep_k@8-3]",
                      OPS + "test_conv_pipelined_kernels[sim-skip@8-3]", OPS + "test_conv_pipelined_kernels[sim-block_tail@8-3]",
                      OPS + "test_conv_pipelined_kernels[sim-gn_fused@8-9]", OPS + "test_conv_split_k[sim-natural@8]"],
    "conv_pipe128.hip": [OPS + "test_conv_pipelined_128cout_kernel[sim-gn_fused@8-4]", OPS + "test_conv_pipelined_128cout_kernel[sim-block_tail@8-4]",
                         OPS + "test_conv_pipelined_128cout_kernel[sim-deep_k-4]"],
    "conv_duo.hip": [OPS + "test_conv_pipelined_128cout_kernel[sim-gn_fused@8-5]", OPS + "test_conv_pipelined_128cout_kernel[sim-block_tail@8-5]",
                     OPS + "test_conv_pipelined_128cout_kernel[sim-deep_k-5]"],
    "conv_thin.hip": [OPS + "test_conv_thin_input_kernel[sim-stem_ragged-dtype0]", OPS + "test_conv_thin_input_kernel[sim-combine_ragged-dtype1]",
                      OPS + "test_conv_group_thin_input_equals_own_launches[sim-1-True]"],
    "conv_narrow.hip": [OPS + "test_conv_narrow_output_kernel[sim-c256_gn_walk-dtype0]", OPS + "test_conv_narrow_output_kernel[sim-c256_two_planes-dtype1]",
                        OPS + "test_conv_group_narrow_output_equals_own_launches[sim-256-True-3]"],
    "attention.hip": [OPS + "test_fused_attention_key_split[sim-64-260-8-dt0-0.008]", OPS + "test_attention_group_equals_own_unsplit_calls[sim-dt0]",
                      OPS + "test_fused_attention[sim-256-70-dt1-0.0015]",
                      # attention_f32_kernel's own staging and barriers, up to nine key tiles and three query blocks; the CT = 4 body, split
                      "tests/test_attention_edges.py::test_rows_within_the_plain_restatement[sim-random-fp32-128-S1]",
                      "tests/test_attention_edges.py::test_rows_within_the_plain_restatement[sim-flat-fp16-128-S2]"],
    "norm_resample.hip": [OPS + "test_groupnorm_fir_fused[sim-shape1-2-dtype1]", OPS + "test_groupnorm_fir_fused[sim-shape4-1-dtype1]",
                          OPS + "test_groupnorm_fir_fused_two_inputs[sim-shape0-24-2-dtype1]", OPS + "test_groupnorm_silu[sim-24-16-dtype1]"],
    "pyramid.hip": [OPS + "test_pyramids_equal_their_chains[sim-dtype1]"],
    "elementwise.hip": [OPS + "test_softmax_rows[sim-dtype1]", OPS + "test_pack_input_and_output_head[sim-dtype1]"],
    "sde.hip": [OPS + "test_sde_steps_vs_oracle[sim]", "tests/test_valid_loss.py::test_dsm_loss_kernel[sim-mse-2-263-2001]",
                "tests/test_valid_loss.py::test_pair_loss_kernel[sim-True-mae-2-263-2001]",
                "tests/test_ode_kernels.py::test_rk_scaled_sumsq_rows_vs_reference[sim-3-259]", "tests/test_ode_kernels.py::test_batch_l2norm[sim]"],
    "spectral.hip": [OPS + "test_stft_batched_ragged_vs_oracle[sim]", "tests/test_resample.py::test_ragged_rows_equal_their_own_calls[sim-160-441-3000]"],
    "stoi.h": ["tests/test_stoi.py::test_kernel_vs_restatement_at_10k[sim]", "tests/test_stoi.py::test_resampler_vs_scipy[sim-a16k]"],
    "align.h": ["tests/test_align.py::test_planted_delays[sim-1000]", "tests/test_align.py::test_lags_per_thread_change_no_bit[sim-2]",
                "tests/test_align.py::test_sosfilt_ragged_batch_equals_one_row_calls[sim-3-22]", "tests/test_align.py::test_shift_rows[sim-1030]"],
    "bss.h": ["tests/test_bss_sdr.py::test_correlations_bit_equal[sim-512]", "tests/test_bss_sdr.py::test_sdr_and_filter_against_cpu_solvers[sim-ar2-4097-64]"],
    "metrics.h": ["tests/test_metrics.py::test_energy_rows_do_not_depend_on_the_batch[sim]", "tests/test_metrics.py::test_lsd_ragged_rows_equal_their_own_calls[sim]"],
    # no LDS of their own today, listed so that their kernels run under skew as well
    "longform.h": ["tests/test_long_form.py::test_several_recordings_in_one_launch[sim-recs1]"],
    "tasnet.h": ["tests/test_convtasnet.py::test_depthwise_kernel[sim-96-64-4-dtype1]", "tests/test_convtasnet.py::test_pointwise_kernel[sim-8-32-7-True-dtype1]",
                 "tests/test_convtasnet.py::test_encoder_kernel[sim-3-1037-64-32-dtype1]", "tests/test_convtasnet.py::test_decoder_kernel[sim-7-64-32-dtype1]"],
    # one tiny whole-network forward (bf16: the MFMA kernels): the program interpreter and the fused-statistics chain
    "program.hip": [NET + "test_tiny_net_vs_reference_golden[sim-dtype1-tiny4]"],
}
SELECTION = [t for tests in COVERAGE.values() for t in tests]
# the LDS-DMA families again with copies that land late (first / last only)
DMA_FAMILIES = ["conv_igemm.hip", "conv_pipe.hip", "conv_pipe128.hip", "conv_duo.hip"]
SELECTION_LATE = [t for f in DMA_FAMILIES for t in COVERAGE[f]]


def test_every_kernel_file_with_lds_has_a_case():
    csrc = os.path.join(ROOT, "storm_amd", "csrc")
    with_lds = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))
                      and re.search(r"__shared__|smem", open(os.path.join(csrc, f)).read()))
    assert with_lds, "no kernel sources found"
    missing = [f for f in with_lds if not COVERAGE.get(f)]
    assert not missing, f"kernel files that declare LDS but have no case in COVERAGE (tests/test_sim_schedules.py): {missing}"
    assert len(set(SELECTION)) == len(SELECTION)


def _inner(tests, waves, dma):
    env = dict(_env(waves, dma), STORM_TEST_WORKERS="2")
    r = subprocess.run([sys.executable, "-m", "pytest"] + [os.path.join(ROOT, t) for t in tests] + ["-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == len(tests) and "skipped" not in r.stdout, r.stdout[-1000:]    # every id exists and ran


@pytest.mark.parametrize("waves,dma", [("reverse", ""), ("first", ""), ("last", ""), ("first", "late"), ("last", "late")],
                         ids=["reverse", "first", "last", "first+late_dma", "last+late_dma"])
def test_real_kernels_under_skewed_wave_schedules(waves, dma):
    """A failure here is a finding about the kernel (a missing barrier, a wait that is one too few, a slot index), not about
    the simulator: replay it with STORM_SIM_WAVES / STORM_SIM_DMA set to this case's values."""
    _inner(SELECTION_LATE if dma else SELECTION, waves, dma)
