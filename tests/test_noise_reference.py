"""The in-kernel Philox noise against an independent reference (tests/philox_ref.py), on both backends.

Every seeded result draws its noise inside the SDE kernels (complex_normal() in csrc/sde.hip: Philox4x32-10 keyed by the seed,
counter = (element index, offset), Box-Muller on the first two output words).  The other noise tests compare kernel output with
kernel output; here the generator meets a numpy Philox written from the published definition and a float64 Box-Muller:

  a. storm_complex_randn element by element, over seeds and offsets that use both words of the key and of the offset, lengths
     around the 256-thread block, the per-row-key form, and a row long enough to go round the grid-stride loop a second time;
  b. the four corners of the uniform map (u1 smallest / exactly 1, u2 exactly 1 / smallest);
  c. every entry point that draws: the call that generates its noise equals the same call given the reference draw as z.  A kernel
     that reads another counter, offset or key word than the documented one misses by O(1), not by rounding: that is what these
     cases are for (the bound they hold is ~1e-6);
  d. the samplers: a seeded run equals the run whose noise_fn hands out the reference draws of offsets 1, 2, 3, ... in call order.

Tolerance (a, b).  Integer part, uniforms and angle are exact, so kernel and reference differ by the rounding of logf, sqrtf,
sincosf and one multiply per component.  No accuracy table of the device math library is at hand, so the tolerance is a
measurement against the reference, in fp32 ulps of the reference component, with a 4 x margin for the difference between two math
libraries and a cap of 16 ulp that is a condition, not a measurement (a defect in the integer part moves outputs by ~2^23 ulp):

    measured maxima over case (a):   host simulation (glibc)  2.21 ulp        MI355X (device math library)  3.25 ulp
    ULP_TOL = min(16, 4 * max of the two) = 13 ulp
    (host: seed 1234; device: the 2048 * 256 + 7 row, its other cases 2.32 .. 2.88; rel-L2 of a draw 4e-8 .. 9e-8 on both; the four
    corners 0 .. 0.83 ulp on both backends, bit-equal to each other)

(c) and (d) propagate that bound: a generated draw differs from the injected one - the reference rounded once to complex64 - by at
most DZ = (ULP_TOL + 0.5) ulp per component, and an update x = x_mean + scale_b z moves by scale_b DZ plus one ulp of the result.

The one part of the counter the suite does not reach is the HIGH word of the element index (counter word 1): it is non-zero only
from element 2^32 on, a 32 GiB row.  The high words of the offset and of the seed are reached (offset 2^32 + 5, seeds >= 2^32)."""
import math

import numpy as np
import pytest
import torch

from tests import philox_ref as P
from tests.backend import dev  # noqa: F401
from tests.util import rel_l2

MEASURED_ULP = {"sim": 2.21, "hip": 3.25}                  # maxima of case (a), see the module docstring
ULP_TOL = min(16.0, 4.0 * max(MEASURED_ULP.values()))

SEEDS = [0, 1234, 2 ** 32, 2 ** 40 + 3, 2 ** 62 - 1, 2 ** 63 - 1]
OFFSETS = [0, 1, 5, 2 ** 32 + 5]
LENGTHS = [1, 255, 1000, 256 * 5 + 7]
ROW_SEEDS = [7, 2 ** 40 + 3, 2 ** 63 - 1]
STRIDE_ROW = 2048 * 256                                     # the row launch caps at 2048 blocks of 256 threads
TOP_SEED = 2 ** 64 - 1                                      # `seed` is a uint64_t argument; a row key lies in [0, 2^63) (ops.row_seed_table)
B, N_ROW = 3, 1000
KEY_MODES = [dict(seed=TOP_SEED), dict(row_seeds=ROW_SEEDS)]
DRAW_OFFSETS = [1, 2 ** 32 + 5]


def _np(t):
    return t.detach().cpu().numpy()


def _c64(zref, shape=None):
    """the reference draw rounded once to complex64, as a torch tensor"""
    z = torch.from_numpy(np.ascontiguousarray(zref.astype(np.complex64)))
    return z if shape is None else z.reshape(shape)


def _measure(got, zref):
    """(max ulp deviation, rel-L2) of a generated draw against the reference"""
    return float(P.ulp_dev(_np(got), zref).max()), rel_l2(_np(got).astype(np.complex128), zref)


def _dz(zref):
    """DZ, per component (re, im): how far a generated draw that meets ULP_TOL lies from the reference rounded to complex64"""
    return (ULP_TOL + 0.5) * P.ulp32(zref.real), (ULP_TOL + 0.5) * P.ulp32(zref.imag)


# ---------------------------------------------------------------- the generator itself (no backend)
def test_philox_known_answers():
    """the three Random123 known-answer vectors of Philox4x32-10 (kat_vectors: zero, all ones, the digits of pi)"""
    kat = [((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 2, (0xFFFFFFFF,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for (k0, k1), (c0, c1, c2, c3), want in kat:
        out = P.philox4x32_10(k0 | k1 << 32, c0 | c1 << 32, c2 | c3 << 32)
        assert " ".join(f"{int(w):08x}" for w in out) == want
    keys = [k[0][0] | k[0][1] << 32 for k in kat]                                # the vectorised form gives the same words
    los, his = [k[1][0] | k[1][1] << 32 for k in kat], [k[1][2] | k[1][3] << 32 for k in kat]
    out = P.philox4x32_10(keys, los, his)
    assert [" ".join(f"{int(w[j]):08x}" for w in out) for j in range(3)] == [k[2] for k in kat]


def test_reference_layout():
    """the helpers' key / counter layout: one seed counts through the batch, row keys count within the row"""
    one = P.draw_one_seed(2 ** 40 + 3, 3, 10, 5)
    re, im = P.complex_normal_ref(2 ** 40 + 3, 2 * 10 + 4, 5)
    assert one[2, 4] == re + 1j * im
    rows = P.draw_row_keys(ROW_SEEDS, 10, 5)
    for b, key in enumerate(ROW_SEEDS):
        assert np.array_equal(rows[b], P.draw_one_seed(key, 1, 10, 5)[0])
    assert np.array_equal(P.draw(3, 10, 5, row_seeds=np.array(ROW_SEEDS, dtype=np.int64)), rows)
    u = P.uniform_f32(np.array([0, 0xFF, 0x100, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and u.tolist() == [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, 1.0, 1.0]
    assert P.ulp32(np.array([1.0, 1.5, 2.0, 0.0, -0.75])).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149, 2.0 ** -24]


# ---------------------------------------------------------------- a. complex_randn element by element
@pytest.mark.parametrize("seed", SEEDS)
def test_complex_randn_against_reference(dev, seed):
    """storm_complex_randn(n, seed, offset) == the reference draw of counters 0 .. n - 1, every element, for every offset and length"""
    from storm_amd import ops
    worst_ulp = worst_l2 = 0.0
    for offset in OFFSETS:
        for n in LENGTHS:
            z = ops.complex_randn((n,), dev, seed, offset)
            u, e = _measure(z, P.draw_one_seed(seed, 1, n, offset)[0])
            worst_ulp, worst_l2 = max(worst_ulp, u), max(worst_l2, e)
    print(f"complex_randn seed {seed}: worst rel-L2 vs the numpy Philox + fp64 Box-Muller {worst_l2:.2e}, max deviation {worst_ulp:.2e} ulp")
    assert worst_ulp <= ULP_TOL


def test_complex_randn_rows_against_reference(dev):
    """the rows form: row b is the draw of (key row_seeds[b], counters 0 .. n - 1)"""
    from storm_amd import ops
    keys = torch.tensor(ROW_SEEDS, dtype=torch.int64).to(dev)
    worst_ulp = worst_l2 = 0.0
    for offset in OFFSETS:
        z = ops.complex_randn((B, N_ROW), dev, 0, offset, row_seeds=keys)
        u, e = _measure(z, P.draw_row_keys(ROW_SEEDS, N_ROW, offset))
        worst_ulp, worst_l2 = max(worst_ulp, u), max(worst_l2, e)
    print(f"complex_randn rows: worst rel-L2 vs the reference {worst_l2:.2e}, max deviation {worst_ulp:.2e} ulp")
    assert worst_ulp <= ULP_TOL


def test_stride_loop_row_against_reference(dev):
    """A generated row of 2048 * 256 + 7 elements: the first seven threads go round the grid-stride loop a second time, and what they
    draw there must be the draws of counters 2048 * 256 .. 2048 * 256 + 6 (both key forms)."""
    from storm_amd import ops
    seed, offset, n = 2 ** 40 + 3, 5, STRIDE_ROW + 7
    zref = P.draw_one_seed(seed, 1, n, offset)[0]
    re, im = P.complex_normal_ref(seed, np.arange(STRIDE_ROW, STRIDE_ROW + 7, dtype=np.uint64), offset)
    assert np.array_equal(zref[-7:], re + 1j * im)
    z = ops.complex_randn((n,), dev, seed, offset)
    u, e = _measure(z, zref)
    ut = float(P.ulp_dev(_np(z[-7:]), zref[-7:]).max())
    zr = ops.complex_randn((1, n), dev, 0, offset, row_seeds=torch.tensor([seed], dtype=torch.int64).to(dev))
    ur, _ = _measure(zr[0], zref)
    print(f"complex_randn stride-loop row: rel-L2 vs the reference {e:.2e}, max deviation {max(u, ur):.2e} ulp, second-trip tail {ut:.2e} ulp")
    assert max(u, ur) <= ULP_TOL and ut <= ULP_TOL


# ---------------------------------------------------------------- b. the corners of the uniform map
CORNERS = [(2210430, 0, 0x000000), (7935899, 0, 0xFFFFFF), (5690486, 1, 0xFFFFFF), (26899134, 1, 0x000000)]


@pytest.mark.parametrize("seed,word,top24", CORNERS)
def test_uniform_corners(dev, seed, word, top24):
    """The first draw (idx 0, offset 1) of four seeds found by search with the reference: output word 0 >> 8 == 0 (smallest u1: the
    largest magnitude the generator can emit, sqrt(25 ln 2)), == 0xFFFFFF (+ 0.5f rounds to even: u1 == 1, r == 0, both components
    exactly +-0), word 1 >> 8 == 0xFFFFFF (u2 == 1, theta = fl32(2 pi)) and == 0 (smallest theta)."""
    from storm_amd import ops
    c = P.philox4x32_10(seed, 0, 1)
    assert int(c[word]) >> 8 == top24                       # re-derived, not trusted
    u = float(P.uniform_f32(c[word]))
    assert u == (1.0 if top24 else 2.0 ** -25)
    re, im = P.complex_normal_ref(seed, 0, 1)
    zref = np.array([re + 1j * im])
    if word == 0 and top24 == 0:
        assert abs(abs(zref[0]) - math.sqrt(25 * math.log(2))) < 1e-12
    z = ops.complex_randn((1,), dev, seed, 1)
    assert torch.isfinite(torch.view_as_real(z)).all()
    dev_ulp, e = _measure(z, zref)
    print(f"uniform corner seed {seed}: rel-L2 vs the reference {e:.2e}, max deviation {dev_ulp:.2e} ulp, z = {z[0].item()}")
    assert dev_ulp <= ULP_TOL
    if word == 0 and top24 == 0xFFFFFF:
        assert zref[0] == 0 and float(z.real[0]) == 0.0 and float(z.imag[0]) == 0.0


# ---------------------------------------------------------------- c. every entry point that draws
class _Ouve:
    """OUVESDE's coefficients in float64 (sdes.py of the reference: 200-231)"""
    theta, smin, smax = 1.5, 0.05, 0.5

    def __init__(self, N):
        from storm_amd.sdes import OUVESDE
        self.N, self.ls = N, math.log(self.smax / self.smin)
        self.sde = OUVESDE(self.theta, self.smin, self.smax, N=N)

    def a(self, t):
        return np.full(np.shape(t), self.theta)

    def g(self, t):
        return self.smin * (self.smax / self.smin) ** np.asarray(t, dtype=np.float64) * math.sqrt(2 * self.ls)

    def std(self, t):
        t, th, ls = np.asarray(t, dtype=np.float64), self.theta, self.ls
        return np.sqrt(self.smin ** 2 * np.exp(-2 * th * t) * (np.exp(2 * (th + ls) * t) - 1) * ls / (th + ls))


class _Ouvp:
    """OUVPSDE's coefficients in float64 (sdes.py of the reference: 286-306)"""
    b0, b1, s = 0.1, 2.0, 1

    def __init__(self, N):
        from storm_amd.sdes import OUVPSDE
        self.N = N
        self.sde = OUVPSDE(self.b0, self.b1, self.s, N=N)

    def a(self, t):
        return 0.5 * self.s * (self.b0 + np.asarray(t, dtype=np.float64) * (self.b1 - self.b0))

    def g(self, t):
        return np.sqrt(self.b0 + np.asarray(t, dtype=np.float64) * (self.b1 - self.b0))

    def std(self, t):
        t = np.asarray(t, dtype=np.float64)
        return (1 - np.exp(-0.5 * self.s * t * (t * (self.b1 - self.b0) + 2 * self.b0))) / self.s


T_ROWS = [0.9, 0.5, 0.2]
SNR = 0.5
SCALE_SLACK = 1 + 1e-5            # the kernels' scale is an fp32 number a few roundings from the float64 value used in the bound


def _inputs(dev):
    g = torch.Generator().manual_seed(2024)
    x, y, score = (torch.view_as_complex(0.3 * torch.randn(B, N_ROW, 2, generator=g)).to(dev) for _ in range(3))
    return dict(x=x, y=y, score=score, t=torch.tensor(T_ROWS).to(dev))


def _entry_points():
    """name -> (fn(inputs, **noise keywords) -> (noisy output, x_mean or None), noise scale per row in float64)"""
    from storm_amd import ops
    ve, vp = _Ouve(30), _Ouvp(30)
    t = np.array(T_ROWS)
    ones = np.ones(B)
    pstd = lambda i: vp.sde._std(i["t"].cpu())                              # noqa: E731
    eps = {
        "ouve_prior": (lambda i, **k: (ops.ouve_prior(ve.sde, i["y"], **k), None), ve.std(ones)),
        "ouve_ald_step": (lambda i, **k: ops.ouve_ald_step(ve.sde, i["x"].clone(), i["score"], i["t"], SNR, **k), 2 * SNR * ve.std(t)),
        "sde_prior_rows": (lambda i, **k: (ops.sde_prior_rows(i["y"], pstd(i), **k), None), vp.std(t)),
    }
    for kind in (0, 1):
        eps[f"ouve_predictor_step_k{kind}"] = (lambda i, kind=kind, **k: ops.ouve_predictor_step(
            ve.sde, i["x"].clone(), i["score"], i["y"], i["t"], kind=kind, **k), ve.g(t) * math.sqrt(1 / 30))
        eps[f"sde_predictor_step_rows_k{kind}"] = (lambda i, kind=kind, **k: ops.sde_predictor_step_rows(
            vp.sde, i["x"].clone(), i["score"], i["y"], i["t"].cpu(), kind=kind, **k), vp.g(t) * math.sqrt(1 / 30))
    for v in (ve, vp):
        form = v.sde.MEAN_FORM
        eps[f"sde_perturb_rows_form{form}"] = (lambda i, v=v, **k: (ops.sde_perturb_rows(
            i["x"], i["y"], v.sde.mean_factor_rows(i["t"].cpu()), v.sde._std(i["t"].cpu()), v.sde.MEAN_FORM, **k), None), v.std(t))
    return eps


ENTRY_POINTS = ["ouve_prior", "ouve_ald_step", "ouve_predictor_step_k0", "ouve_predictor_step_k1", "sde_prior_rows",
                "sde_predictor_step_rows_k0", "sde_predictor_step_rows_k1", "sde_perturb_rows_form0", "sde_perturb_rows_form1"]


def _component_excess(got, want, bound_re, bound_im):
    """the worst |got - want| / bound over the components of two complex64 arrays (<= 1: within the bound)"""
    g, w = _np(got).astype(np.complex128), _np(want).astype(np.complex128)
    return float(max((np.abs(g.real - w.real) / bound_re).max(), (np.abs(g.imag - w.imag) / bound_im).max()))


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_point_draws_the_reference_noise(dev, name):
    """The call that draws in the kernel (z=None, seed / offset / row_seeds) against the same call given z = the reference draw of those
    keys: x_mean does not depend on the noise and is bit-equal; the noisy output x = x_mean + scale_b z differs per component by at
    most scale_b DZ plus one ulp of the result.  A kernel that reads another counter, offset or key word than its documentation says
    misses by O(scale_b), about six orders above the bound - that, not the rounding, is what this case is for."""
    fn, scale = _entry_points()[name]
    ins = _inputs(dev)
    worst = worst_l2 = worst_ulp = 0.0
    for keys in KEY_MODES:
        for offset in DRAW_OFFSETS:
            zref = P.draw(B, N_ROW, offset, **keys)
            got, got_mean = fn(ins, offset=offset, **keys)
            inj, inj_mean = fn(ins, z=_c64(zref).to(dev))
            assert torch.isfinite(torch.view_as_real(got)).all()
            if inj_mean is not None:
                assert torch.equal(got_mean, inj_mean), (name, keys, offset)
            dre, dim = _dz(zref)
            w = _np(inj).astype(np.complex128)
            s = scale[:, None] * SCALE_SLACK
            worst = max(worst, _component_excess(got, inj, s * dre + P.ulp32(w.real), s * dim + P.ulp32(w.imag)))
            worst_ulp = max(worst_ulp, _component_excess(got, inj, np.maximum(s * P.ulp32(zref.real), P.ulp32(w.real)),
                                                         np.maximum(s * P.ulp32(zref.imag), P.ulp32(w.imag))))
            worst_l2 = max(worst_l2, rel_l2(got.cpu(), inj.cpu()))
    print(f"{name}: generated vs reference-injected noise, worst rel-L2 {worst_l2:.2e}, max deviation {worst_ulp:.2e} ulp (of the scaled draw or the result, the larger), "
          f"worst |delta| / bound {worst:.2e} (bound from {ULP_TOL + 0.5:.2e} ulp per drawn component)")
    assert worst <= 1.0


@pytest.mark.parametrize("kind", ["mse", "mae"])
def test_dsm_loss_draws_the_reference_noise(dev, kind):
    """storm_dsm_loss_rows re-draws the perturbation's noise: its row sums 0.5 sum rho(score std_b + z) with generated z against the
    same sums with the reference draw injected, relatively.  Bound: a residual component e = s std_b + z moves by d = DZ + ulp(e) (the
    draw, and one rounding of the sum); |e|^2 then moves by 2 |e| d + d^2 and |e| (the complex modulus) by |d|; the fp64 sum adds
    nothing visible and the fp32 result one ulp.  Another counter, offset or key moves a row sum by ~1 / sqrt(n) of itself (O(1)
    per element)."""
    from storm_amd import ops
    vp = _Ouvp(30)
    ins = _inputs(dev)
    std = vp.sde._std(torch.tensor(T_ROWS)).to(dev)
    sd = _np(std).astype(np.float64)[:, None]
    s = _np(ins["score"]).astype(np.complex128)
    worst = worst_rel = worst_ulp = 0.0
    for keys in KEY_MODES:
        for offset in DRAW_OFFSETS:
            zref = P.draw(B, N_ROW, offset, **keys)
            got = _np(ops.dsm_loss_rows(ins["score"], std, kind=kind, offset=offset, **keys)).astype(np.float64)
            inj = _np(ops.dsm_loss_rows(ins["score"], std, z=_c64(zref).to(dev), kind=kind)).astype(np.float64)
            e = s * sd + zref
            dre, dim = _dz(zref)
            dre, dim = dre + P.ulp32(e.real), dim + P.ulp32(e.imag)
            if kind == "mse":
                moved = 2 * np.abs(e.real) * dre + dre ** 2 + 2 * np.abs(e.imag) * dim + dim ** 2
            else:
                moved = np.hypot(dre, dim)
            bound = 0.5 * moved.sum(axis=1) + P.ulp32(inj)
            assert np.isfinite(got).all() and (inj > 0).all()
            worst = max(worst, float((np.abs(got - inj) / bound).max()))
            worst_rel = max(worst_rel, float((np.abs(got - inj) / inj).max()))
            worst_ulp = max(worst_ulp, float(P.ulp_dev(got, inj).max()))
    print(f"dsm_loss_rows {kind}: generated vs reference-injected noise, worst row rel-L2 {worst_rel:.2e}, max deviation {worst_ulp:.2e} ulp "
          f"of the row sum, worst |delta| / bound {worst:.2e}")
    assert worst <= 1.0


def test_langevin_pair_draws_the_reference_noise(dev):
    """The Langevin corrector's pair complex_randn -> langevin_step against langevin_step on the reference draw.  Here the step size
    itself follows the noise (step = 2 r^2, noise scale 2 r, r = snr mean_b |z_b| / mean_b |score_b|, correctors.py:53-55), so x_mean
    moves too: with |delta mean_b |z_b||  <= mean_b |DZ_b| (l2 norms over the row) and four fp32 operations on the way to r,
    delta r / r <= that / mean_b |z_b| + 4 * 2^-23; per component  |delta x_mean| <= delta(step) |s| + ulp,
    |delta x| <= |delta x_mean| + 2 r DZ + 2 delta(r) |z| + ulp."""
    from storm_amd import ops
    ins = _inputs(dev)
    s = _np(ins["score"]).astype(np.complex128)
    gs = np.sqrt((np.abs(s) ** 2).sum(axis=1)).mean()
    worst = worst_l2 = worst_ulp = 0.0
    for keys in KEY_MODES:
        for offset in DRAW_OFFSETS:
            zref = P.draw(B, N_ROW, offset, **keys)
            rows = torch.tensor(keys["row_seeds"], dtype=torch.int64).to(dev) if "row_seeds" in keys else None
            z = ops.complex_randn((B, N_ROW), dev, keys.get("seed", 0), offset, row_seeds=rows)
            got, got_mean = ops.langevin_step(ins["x"].clone(), ins["score"], z, SNR)
            inj, inj_mean = ops.langevin_step(ins["x"].clone(), ins["score"], _c64(zref).to(dev), SNR)
            dre, dim = _dz(zref)
            gz = np.sqrt((np.abs(zref) ** 2).sum(axis=1)).mean()
            dgz = np.sqrt((dre ** 2 + dim ** 2).sum(axis=1)).mean()
            r = SNR * gz / gs
            dr = r * (dgz / gz + 4 * 2.0 ** -23) * SCALE_SLACK
            dstep = 2 * (2 * r * dr + dr ** 2)
            wm, w = _np(inj_mean).astype(np.complex128), _np(inj).astype(np.complex128)
            mre, mim = dstep * np.abs(s.real) + P.ulp32(wm.real), dstep * np.abs(s.imag) + P.ulp32(wm.imag)
            worst = max(worst, _component_excess(got_mean, inj_mean, mre, mim))
            worst = max(worst, _component_excess(got, inj, mre + 2 * r * SCALE_SLACK * dre + 2 * dr * np.abs(zref.real) + P.ulp32(w.real),
                                                 mim + 2 * r * SCALE_SLACK * dim + 2 * dr * np.abs(zref.imag) + P.ulp32(w.imag)))
            worst_ulp = max(worst_ulp, _component_excess(got, inj, np.maximum(2 * r * P.ulp32(zref.real), P.ulp32(w.real)),
                                                         np.maximum(2 * r * P.ulp32(zref.imag), P.ulp32(w.imag))))
            worst_l2 = max(worst_l2, rel_l2(got.cpu(), inj.cpu()))
    print(f"complex_randn -> langevin_step: generated vs reference noise, worst rel-L2 {worst_l2:.2e}, max deviation {worst_ulp:.2e} ulp (of the "
          f"scaled draw or the result, the larger), worst |delta| / bound {worst:.2e}")
    assert worst <= 1.0


# ---------------------------------------------------------------- d. the samplers' draw sequence
SAMPLER_SEED = 2 ** 40 + 3
N_STEPS = 3
EPS = 0.03
RUNS = {"ouve-pc-reverse_diffusion-ald": ("ouve", "reverse_diffusion", "ald"),
        "ouve-pc-euler_maruyama-langevin": ("ouve", "euler_maruyama", "langevin"),
        "ouve-pc-reverse_diffusion-none": ("ouve", "reverse_diffusion", "none"),
        "ouvp-pc-reverse_diffusion-langevin": ("ouvp", "reverse_diffusion", "langevin")}


def _y(dev):
    return (torch.randn(2, 1, 8, 16, dtype=torch.complex64, generator=torch.Generator().manual_seed(0)) * 0.3).to(dev)


def _recording_score(trace):
    """the analytic score -(x - y); every state it is asked about goes to `trace`"""
    def score(x, t, y, **kw):
        trace.append(_np(x).astype(np.complex128).reshape(x.shape[0], -1))
        return -(x - y)
    return score


def _maxc(a):
    return float(max(np.abs(a.real).max(), np.abs(a.imag).max()))


def _pc_bound(v, corr, y, zrefs, trace, result):
    """The bound on |seeded run - reference-injected run| per component of a PC run with the score s = y - x, propagated draw by draw.
    Every update is x <- x + c (y - x) + b z with per-row scalars: an error E of the state becomes |1 - c| E + b DZ.
      prior                       x = y + std(T) z
      ald corrector               c = 2 (snr std(t))^2, b = 2 snr std(t)
      langevin corrector          c = 2 r^2, b = 2 r, r = snr mean_b |z_b| / mean_b |s_b|: r follows the draw and the state,
                                  delta r / r <= (sqrt(2 n) DZ) / mean |z_b| + (sqrt(2 n) E) / mean |s_b| + 4 * 2^-23  (an l2 norm of 2 n
                                  components moves by at most sqrt(2 n) times the largest move of one), adding delta(c) |s| + delta(b) |z|
      predictor (both kinds)      c = (g(t)^2 - a(t)) / N, b = g(t) / sqrt(N); the run returns the last x_mean, before b z is added
    and each update rounds a handful of fp32 operations on numbers no larger than the largest state component: 8 ulp of that per
    update (RND) for the two runs together.  The magnitudes (|s|, |z|, r) are read from the reference-injected run."""
    yv = _np(y).astype(np.complex128).reshape(y.shape[0], -1)
    n = yv.shape[1]
    rnd = 8 * float(P.ulp32(max(_maxc(yv), _maxc(result), max(_maxc(x) for x in trace))))
    dzmax = [float(max(d.max() for d in _dz(z))) for z in zrefs]
    ts = np.linspace(1.0, EPS, N_STEPS)
    draws, calls = iter(range(1, len(zrefs))), iter(trace)
    E = float(v.std(1.0)) * SCALE_SLACK * dzmax[0] + rnd
    Em = E
    for t in ts:
        if corr != "none":
            x, k = next(calls), next(draws)
            if corr == "ald":
                b = 2 * SNR * float(v.std(t)) * SCALE_SLACK
                E = abs(1 - b * b / 2) * E + b * dzmax[k] + rnd
            else:
                s, z = yv - x, zrefs[k]
                gs, gz = np.sqrt((np.abs(s) ** 2).sum(axis=1)).mean(), np.sqrt((np.abs(z) ** 2).sum(axis=1)).mean()
                r = SNR * gz / gs
                rel = math.sqrt(2 * n) * dzmax[k] / gz + math.sqrt(2 * n) * E / gs + 4 * 2.0 ** -23
                assert rel < 1e-3
                dr = r * rel * 1.01                                       # (1 / (1 - delta gs / gs) <= 1.01)
                E = abs(1 - 2 * r * r) * E + 2 * (2 * r * dr + dr * dr) * _maxc(s) + 2 * r * dzmax[k] + 2 * dr * _maxc(z) + rnd
        next(calls)
        k = next(draws)
        g, a = float(v.g(t)), float(v.a(t))
        Em = abs(1 - (g * g - a) / N_STEPS) * E * SCALE_SLACK + rnd
        E = Em + g * math.sqrt(1 / N_STEPS) * SCALE_SLACK * dzmax[k] + rnd
    assert next(calls, None) is None and next(draws, None) is None
    return Em


def _spy_offsets(monkeypatch):
    from storm_amd.sampling import NoiseSource
    handed, orig = [], NoiseSource.next

    def spy(self, like):
        out = orig(self, like)
        handed.append(out[2])
        return out
    monkeypatch.setattr(NoiseSource, "next", spy)
    return handed


@pytest.mark.parametrize("run", list(RUNS))
def test_pc_sampler_draw_sequence(dev, run, monkeypatch):
    """get_pc_sampler(seed = 2^40 + 3), N = 3, one corrector step, against the same sampler whose noise_fn hands out the reference draws
    of offsets 1, 2, 3, ... in call order: the prior first, then per step the corrector's draw and then the predictor's.  The PC
    sampler draws for every predictor step, the last one included (it returns that step's x_mean, but the draw is made):
    1 + N (corrector_steps + 1) calls, and the seeded run's NoiseSource hands out exactly the offsets 1 .. that, each once."""
    from storm_amd.sampling import get_pc_sampler
    kind, pred, corr = RUNS[run]
    v = _Ouve(N_STEPS) if kind == "ouve" else _Ouvp(N_STEPS)
    y = _y(dev)
    n_draws = 1 + N_STEPS * ((corr != "none") + 1)
    zrefs = [P.draw_one_seed(SAMPLER_SEED, 2, y[0].numel(), k) for k in range(1, n_draws + 1)]
    calls, trace = [], []

    def noise_fn():
        calls.append(len(calls) + 1)
        return _c64(zrefs[len(calls) - 1], y.shape)
    kw = dict(sde=v.sde, y=y, eps=EPS, snr=SNR, corrector_steps=1)
    want, nfe = get_pc_sampler(pred, corr, score_fn=_recording_score(trace), noise_fn=noise_fn, **kw)()
    assert len(calls) == n_draws and nfe == n_draws - 1
    handed = _spy_offsets(monkeypatch)
    got, _ = get_pc_sampler(pred, corr, score_fn=lambda x, t, yy, **k: -(x - yy), seed=SAMPLER_SEED, **kw)()
    assert handed == list(range(1, n_draws + 1))
    assert torch.isfinite(torch.view_as_real(got)).all()
    w = _np(want).astype(np.complex128)
    bound = _pc_bound(v, corr, y, zrefs, trace, w)
    worst = _component_excess(got, want, bound, bound)
    print(f"{run}: seeded run vs reference draws through noise_fn, rel-L2 {rel_l2(got.cpu(), want.cpu()):.2e}, "
          f"worst |delta| / bound {worst:.2e} (bound {bound:.2e})")
    assert worst <= 1.0


def test_pc_sampler_row_seeds_draw_sequence(dev, monkeypatch):
    """get_pc_sampler(row_seeds=) (reverse diffusion + ald, N = 3) against a hand-rolled loop over the same kernels that is fed the
    per-row reference draws of offsets 1, 2, ... through their z= arguments (noise_fn cannot be combined with row_seeds)."""
    from storm_amd import ops
    from storm_amd.sampling import get_pc_sampler
    v = _Ouve(N_STEPS)
    y = _y(dev)
    keys = ROW_SEEDS[1:]
    n_draws = 1 + 2 * N_STEPS
    zrefs = [P.draw_row_keys(keys, y[0].numel(), k) for k in range(1, n_draws + 1)]
    zs = iter(_c64(z, y.shape).to(dev) for z in zrefs)
    trace = []
    score = _recording_score(trace)
    x = ops.ouve_prior(v.sde, y, z=next(zs))
    for t in torch.linspace(1, EPS, N_STEPS):
        vec_t = torch.full((2,), float(t)).to(dev)
        x, _ = ops.ouve_ald_step(v.sde, x, score(x, vec_t, y), vec_t, SNR, z=next(zs))
        x, want = ops.ouve_predictor_step(v.sde, x, score(x, vec_t, y), y, vec_t, kind=0, z=next(zs))
    assert next(zs, None) is None
    handed = _spy_offsets(monkeypatch)
    got, nfe = get_pc_sampler("reverse_diffusion", "ald", sde=v.sde, score_fn=lambda x, t, yy, **k: -(x - yy), y=y, eps=EPS, snr=SNR,
                              corrector_steps=1, row_seeds=keys)()
    assert handed == list(range(1, n_draws + 1)) and nfe == n_draws - 1
    w = _np(want).astype(np.complex128)
    bound = _pc_bound(v, "ald", y, zrefs, trace, w)
    worst = _component_excess(got, want, bound, bound)
    print(f"row_seeds reverse_diffusion + ald: sampler vs hand-rolled loop on the per-row reference draws, rel-L2 "
          f"{rel_l2(got.cpu(), want.cpu()):.2e}, worst |delta| / bound {worst:.2e} (bound {bound:.2e})")
    assert worst <= 1.0


def test_ode_sampler_prior_draw(dev, monkeypatch):
    """get_ode_sampler(seed = 2^40 + 3) draws once - the prior, offset 1; its final denoising step is noise-free - and equals the run
    whose noise_fn returns the reference draw.  Bound: the start states differ by E0 = std(T) DZ + RND.  With s = y - x the flow is
    d(x - y)/dt = -(theta - g^2 / 2) (x - y), integrated from T down to eps: a difference grows by at most exp(theta (T - eps)).  Both
    runs take the same steps (asserted: same evaluation count), so they apply the same linear Runge-Kutta map, whose factor is the
    flow's to the solver's tolerance (1e-5; 1 % allowed); every right-hand side adds RND, carried to the end by at most the same
    factor; the noise-free reverse-diffusion step multiplies by |1 - (g(eps)^2 - theta) / N|."""
    from storm_amd.sampling import get_ode_sampler
    v = _Ouve(N_STEPS)
    y = _y(dev)
    zref = P.draw_one_seed(SAMPLER_SEED, 2, y[0].numel(), 1)
    calls, trace = [], []

    def noise_fn():
        calls.append(1)
        return _c64(zref, y.shape)
    want, nfe_want = get_ode_sampler(v.sde, _recording_score(trace), y=y, eps=EPS, noise_fn=noise_fn)()
    assert len(calls) == 1
    handed = _spy_offsets(monkeypatch)
    got, nfe = get_ode_sampler(v.sde, lambda x, t, yy, **k: -(x - yy), y=y, eps=EPS, seed=SAMPLER_SEED)()
    assert handed == [1] and nfe == nfe_want
    w = _np(want).astype(np.complex128)
    rnd = 8 * float(P.ulp32(max(_maxc(w), max(_maxc(x) for x in trace))))
    growth = math.exp(v.theta * (1 - EPS)) * 1.01
    e0 = float(v.std(1.0)) * SCALE_SLACK * float(max(d.max() for d in _dz(zref))) + rnd
    bound = (e0 + len(trace) * rnd) * growth * abs(1 - (float(v.g(EPS)) ** 2 - v.theta) / N_STEPS) + rnd
    worst = _component_excess(got, want, bound, bound)
    print(f"ode sampler: seeded run vs the reference prior draw through noise_fn, nfev {nfe}, rel-L2 {rel_l2(got.cpu(), want.cpu()):.2e}, "
          f"worst |delta| / bound {worst:.2e} (bound {bound:.2e})")
    assert worst <= 1.0
