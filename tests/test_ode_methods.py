"""solve_ivp's RK23 and DOP853 on the device: the tableaux, the wide kernels (up to 13 stages, the paired error sums), the step
controller against scipy.integrate.solve_ivp(method=M), per-row control, the reference's own runs (fixture F25) and the surface.

The scaffold is tests/test_ode_kernels.py: its numpy restatement of scipy's rk_step, its derived bounds and its `bites` (every
comparison is shown to be able to fail).  What is new here is designed around one fact: DOP853's order-8 error estimate can sit in
the fp32 rounding noise of the right-hand side, where its step sequence is decided by that noise and cannot be asked of another
implementation.  The controller cases therefore first show, with scipy alone, that the case does not hinge on rounding (the same nfev
with the right-hand side in complex64 and in complex128) and is accurate (2.5e-4 from a 1e-12 solution); fixture F25 keeps only cases
that pass the first condition on the reference.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ode_method_cases as OC
from tests.backend import dev  # noqa: F401
from tests.test_ode_kernels import (ATOL, ROW_CASES, RTOL, SUM_CASES, U64, GRID_CAP, _c128, _check_sums, _col, _combine_defects, _crandn, _ivp_case,
                                    _last_block_missing, _rv, _sum_terms, bites, bits_equal, magnitude, ref_combine, ref_scaled_sumsq)
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_TERMS = 13                                                           # STORM_RK_MAX_TERMS
METHODS = ["RK23", "DOP853"]


def tableau(method):
    from storm_amd.sampling import ode
    return ode.TABLEAUX[method]


# ---------------------------------------------------------------- 1. the tableaux are scipy's ------------------------------
def test_tableaux_are_scipys():
    """No backend: ode.py's RK23 and DOP853 records equal scipy's class attributes exactly (literals in the product, which does not
    import scipy), the exponents are the solver's, and ode.error_norm is DOP853._estimate_error_norm to 1e-14"""
    from scipy.integrate._ivp import rk

    from storm_amd.sampling import ode
    fun = lambda t, y: -y                                                # noqa: E731
    for tb, cls in ((ode.RK23, rk.RK23), (ode.DOP853, rk.DOP853), (ode.RK45, rk.RK45)):
        ns = cls.n_stages
        assert (tb.name, tb.n_stages, tb.order, tb.error_estimator_order) == (cls.__name__, ns, cls.order, cls.error_estimator_order)
        assert cls.C.shape == (ns,) and cls.B.shape == (ns,) and cls.A.shape[0] == ns
        assert np.array_equal(np.array(tb.C, dtype=np.float64), cls.C) and np.array_equal(np.array(tb.B, dtype=np.float64), cls.B)
        assert len(tb.A) == ns
        for s in range(ns):
            assert len(tb.A[s]) == s and np.array_equal(np.array(tb.A[s], dtype=np.float64), cls.A[s][:s]) and not cls.A[s][s:].any()
        rows = (cls.E5, cls.E3) if cls is rk.DOP853 else (cls.E,)
        assert len(tb.E) == len(rows)
        for mine, theirs in zip(tb.E, rows):
            assert theirs.shape == (ns + 1,) and np.array_equal(np.array(mine, dtype=np.float64), theirs)
        solver = cls(fun, 1.0, np.ones(3, dtype=np.complex128), 0.03, rtol=RTOL, atol=ATOL)
        assert tb.error_exponent == solver.error_exponent
        assert tb.wide == (ns + 1 > 7)
    assert set(ode.TABLEAUX) == {"RK45", "RK23", "DOP853"}
    import ast
    tree = ast.parse(open(ode.__file__).read())
    imported = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    imported |= {(n.module or "").split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level == 0}
    assert "scipy" not in imported
    # the DOP853 norm from the two row sums
    rng = np.random.default_rng(8)
    n = 41
    solver = rk.DOP853(fun, 1.0, np.ones(n, dtype=np.complex128), 0.03, rtol=RTOL, atol=ATOL)
    for trial in range(4):
        K = rng.standard_normal((13, n)) + 1j * rng.standard_normal((13, n))
        scale = ATOL + RTOL * np.abs(rng.standard_normal(n))
        h = -0.01 * (trial + 1)
        want = solver._estimate_error_norm(K, h, scale)
        s5 = float((np.abs(K.T @ rk.DOP853.E5) ** 2 / scale ** 2).sum())
        s3 = float((np.abs(K.T @ rk.DOP853.E3) ** 2 / scale ** 2).sum())
        got = ode.error_norm(ode.DOP853, (s5, s3), h, n)
        assert want > 0 and abs(got - want) <= 1e-14 * want, (got, want)
        assert abs(ode.error_norm(ode.DOP853, (s5, 0.0), h, n) - want) > 1e-6 * want      # (the E3 sum matters)
    assert ode.error_norm(ode.DOP853, (0.0, 0.0), -0.01, n) == 0.0 == solver._estimate_error_norm(np.zeros((13, n)), -0.01, np.ones(n))
    # one estimator: sqrt(sum / n), h already applied by the kernel
    assert ode.error_norm(ode.RK23, (8.0,), -0.5, 2) == 2.0


# ---------------------------------------------------------------- coefficients and inputs ---------------------------------
_RND13 = [0.31, -0.57, 0.83, -0.29, 0.47, -0.91, 0.63, -0.37, 0.71, -0.43, 0.59, -0.77, 0.53]      # no zero: a skipped K[j] would be seen
_RND13B = [-0.61, 0.27, 0.39, -0.87, 0.23, 0.67, -0.33, 0.81, -0.49, 0.93, -0.21, 0.41, -0.73]


def dop_row(nt):
    """DOP853's own row with nt terms: A[nt] (stages 1..11), B (12), E5 (13).  Its B and E rows are zero at indices 1..4"""
    tb = tableau("DOP853")
    return list(tb.A[nt]) if nt <= 11 else (list(tb.B) if nt == 12 else list(tb.E[0]))


def rk23_row(nt):
    tb = tableau("RK23")
    return list(tb.A[nt]) if nt <= 2 else (list(tb.B) if nt == 3 else list(tb.E[0]))


def rnd_row(nt):
    return _RND13[:nt]


ROW_SETS = [("DOP853", dop_row, range(1, 14)), ("RK23", rk23_row, range(1, 5)), ("non-zero", rnd_row, range(1, 14))]


@functools.lru_cache(maxsize=None)
def wide_case(B, n):
    """(x, xb complex128 [B, n], 13 stages complex64, one negative step size per row, row 1's = 0 when there is one); never written to"""
    g = torch.Generator().manual_seed(8000 + 131 * B + n)
    x, xb = _crandn(g, B, n, dtype=torch.complex128) * 1.3, _crandn(g, B, n, dtype=torch.complex128) * 1.3
    K = tuple(_crandn(g, B, n) for _ in range(MAX_TERMS))
    h = [-0.003 * (1 + b % 7) - 1e-4 * b for b in range(B)]
    if B > 1:
        h[1] = 0.0
    return x, xb, K, h


# ROW_CASES' rows are all of odd length; an even row takes the 16-byte path (two complex elements per thread): one block + a
# partial one of PAIRS, and across the 128-row split
WIDE_ROW_CASES = ROW_CASES + [(3, 2 * 259), (130, 4)]


# ---------------------------------------------------------------- 2. the wide stage kernel ---------------------------------
def _check_wide_combine(dev, x, K, h, nt, c, want_rows=False):
    from storm_amd import ops
    xd, Kd = x.to(dev), [k.to(dev) for k in K[:nt]]
    o64, o32 = ops.rk_combine_rows_wide(xd, Kd, c, h, want64=True)
    only32 = ops.rk_combine_rows_wide(xd, Kd, c, h)
    ref = ref_combine(x, K[:nt], c, h)
    bound = 2 * (nt + 1) * U64 * magnitude(x, K[:nt], c, h)             # (test_ode_kernels: one rounding per fma on either side)
    err = np.abs(_rv(_c128(o64)) - _rv(ref))
    assert (err <= bound).all(), (nt, float((err / bound).max()))
    if all(v != 0 for v in c[-1:]):
        _combine_defects(x, K[:nt], c, h, ref, bound)
    assert bits_equal(o32, o64.to(torch.complex64)) and bits_equal(only32, o32)
    for b, hb in enumerate(h):
        if hb == 0:
            assert bits_equal(o64[b], x[b])
    if nt <= 7:
        e64, e32 = ops.rk_combine_rows(xd, Kd, c, h, want64=True)
        assert bits_equal(o64, e64) and bits_equal(o32, e32), nt
    if want_rows:
        for b in range(x.shape[0]):
            a64, a32 = ops.rk_combine_rows_wide(xd[b:b + 1], [k[b:b + 1] for k in Kd], c, h[b:b + 1], want64=True)
            assert bits_equal(a64, o64[b:b + 1]) and bits_equal(a32, o32[b:b + 1]), b
    return float((err / bound).max())


@pytest.mark.parametrize("B,n", WIDE_ROW_CASES)
def test_rk_combine_rows_wide_vs_reference(dev, B, n):
    """out64 within 2 (n_terms + 1) 2^-53 (|x| + |h| sum |c_j| |K_j|) per component, out32 its rounding, the h = 0 row untouched, every row
    bit-equal to its own B = 1 call, and for n_terms <= 7 the bits of rk_combine_rows; n_terms 1..13 with DOP853's and RK23's own rows
    and with non-zero coefficients (a dropped last term bites wherever that term's coefficient is not zero)"""
    x, _, K, h = wide_case(B, n)
    assert 0.0 in h and all(v <= 0 for v in h) and len(set(h)) > 2
    worst = 0.0
    for name, row, terms in ROW_SETS:
        for nt in terms:
            worst = max(worst, _check_wide_combine(dev, x, K, h, nt, row(nt), want_rows=(nt in (4, 12, 13))))
    print(f"rk_combine_rows_wide [{B}, {n}]: worst error {worst:.3g} of the bound (bound = 2 (n_terms + 1) 2^-53 magnitude)")


def test_rk_combine_rows_wide_pair_path(dev):
    """the two-elements-per-thread path: (a) a row of 2 (2048 * 256 + 7) elements - the last 7 pairs are written in the grid-stride loop's
    second round; (b) stages that start 8 bytes off a 16-byte boundary take the one-element path: the same bits as from aligned copies"""
    from storm_amd import ops
    B, n = 1, 2 * (GRID_CAP * 256 + 7)
    g = torch.Generator().manual_seed(78)
    x, K, h = _crandn(g, B, n, dtype=torch.complex128) * 1.3, [_crandn(g, B, n) for _ in range(2)], [-0.0137]
    worst = _check_wide_combine(dev, x, K, h, 2, rnd_row(2))
    print(f"rk_combine_rows_wide [{B}, {n}]: worst error {worst:.3g} of the bound")
    x, _, K, h = wide_case(3, 2 * 259)
    xd = x.to(dev)
    Kd = [k.to(dev) for k in K]
    off = []
    for k in Kd:
        buf = torch.empty(k.numel() + 1, dtype=k.dtype, device=dev)
        buf[1:] = k.reshape(-1)
        off.append(buf[1:].view(k.shape))
        assert off[-1].data_ptr() % 16 == 8 and off[-1].is_contiguous()
    a64, a32 = ops.rk_combine_rows_wide(xd, Kd, rnd_row(13), h, want64=True)
    b64, b32 = ops.rk_combine_rows_wide(xd, off, rnd_row(13), h, want64=True)
    assert bits_equal(a64, b64) and bits_equal(a32, b32)


# ---------------------------------------------------------------- 3. the paired error sums ---------------------------------
def pair_rows(name, nt):
    """two coefficient rows of nt terms: DOP853's E5 / E3 (cut to nt), or two non-zero sets"""
    tb = tableau("DOP853")
    return (list(tb.E[0][:nt]), list(tb.E[1][:nt])) if name == "DOP853" else (_RND13[:nt], _RND13B[:nt])


@pytest.mark.parametrize("B,n", SUM_CASES)
def test_rk_error_pair_rows_vs_reference(dev, B, n):
    """both sums within (n + 64) 2^-53 of the float64 reference, with per-row h (one of them 0) and with h_rows = None (= 1, DOP853's use);
    a missing last block bites; every row bit-equal to its B = 1 call; for n_terms <= 7 each sum is rk_scaled_sumsq_rows' bits"""
    from storm_amd import ops
    x, xb, K, h = wide_case(B, n)
    xn, xbn, Kn = _c128(x), _c128(xb), [_c128(k) for k in K]
    xd, xbd, Kd = x.to(dev), xb.to(dev), [k.to(dev) for k in K]
    worst = 0.0
    small = B * n < 4096                                                 # (the long rows and the 130-row batch: the widths where the paths part)
    for name in ("DOP853", "non-zero"):
        for nt in (range(1, MAX_TERMS + 1) if small else (1, 7, 8, 13)):
            ca, cb = pair_rows(name, nt)
            for hh in ((h, None) if small or nt == 13 else (h,)):
                got = ops.rk_error_pair_rows(xd, xbd, Kd[:nt], ca, cb, hh, ATOL, RTOL)
                assert got.shape == (2, B) and got.dtype == torch.float64
                hv = h if hh is not None else [1.0] * B
                nz = [b for b, v in enumerate(hv) if v != 0]
                for e, c in enumerate((ca, cb)):
                    v = _col(hv, xn) * np.tensordot(np.array(c), np.stack(Kn[:nt]), 1)
                    terms = _sum_terms(v, xn, xbn)
                    ref = terms.sum(-1)
                    assert (ref[[b for b, q in enumerate(hv) if q == 0]] == 0).all() and (ref[nz] > 0).all()
                    worst = max(worst, _check_sums(got[e], ref, n, (name, nt, e, hh is None)))
                    bound = (n + 64) * U64 * ref[nz]
                    bites(ref[nz], _last_block_missing(terms, n)[nz], bound, "last block's share missing")
                    bites(ref[nz], _sum_terms(v, xn, None).sum(-1)[nz], bound, "|xa| alone in the scale")
                    if name == "non-zero":
                        vd = _col(hv, xn) * np.tensordot(np.array(c[:nt - 1]), np.stack(Kn[:nt - 1]), 1) if nt > 1 else 0 * v
                        bites(ref[nz], _sum_terms(vd, xn, xbn).sum(-1)[nz], bound, "last term dropped")
                        other = (cb, ca)[e]
                        bites(ref[nz], _sum_terms(_col(hv, xn) * np.tensordot(np.array(other), np.stack(Kn[:nt]), 1), xn, xbn).sum(-1)[nz], bound,
                              "the other coefficient row")
                    if nt <= 7:
                        assert bits_equal(ops.rk_scaled_sumsq_rows(xd, xbd, Kd[:nt], c, hh, ATOL, RTOL), got[e]), (name, nt, e)
                if nt in (7, 13):
                    for b in (range(B) if B < 8 else (0, 1, 127, 128, B - 1)):
                        alone = ops.rk_error_pair_rows(xd[b:b + 1], xbd[b:b + 1], [k[b:b + 1] for k in Kd[:nt]], ca, cb,
                                                       None if hh is None else hh[b:b + 1], ATOL, RTOL)
                        assert bits_equal(alone, got[:, b:b + 1]), (name, nt, b)
    # xb = NULL: |xa| alone in the scale
    ca, cb = pair_rows("non-zero", 13)
    got = ops.rk_error_pair_rows(xd, None, Kd, ca, cb, None, ATOL, RTOL)
    for e, c in enumerate((ca, cb)):
        _check_sums(got[e], ref_scaled_sumsq(np.tensordot(np.array(c), np.stack(Kn), 1), xn), n, ("no xb", e))
    print(f"rk_error_pair_rows [{B}, {n}]: worst error {worst:.3g} of the bound (bound = (n + 64) 2^-53 relative)")


# ---------------------------------------------------------------- 4. the controller against solve_ivp(method=M) -------------
# (case of _ivp_case, score multiplier, rtol = atol).  DOP853 with the score times 160: at 1e-2 scipy alone needs 314 / 302 evaluations
# (complex64 / complex128 right-hand side) and ends 2.0e-3 from the 1e-12 solution - both conditions fail; at 1e-3 it is 290 / 290
# with 2 rejections, 1.9e-5 away
REJECTION = {"RK23": ("d", 40.0, 1e-5), "DOP853": ("d", 160.0, 1e-3)}


def _toy_problem(case, stiff=None, y_scale=1.0):
    from storm_amd.sdes import OUVESDE
    sde = OUVESDE(1.5, 0.05, 0.5, N=30)
    y, z, eps, st = _ivp_case(case)
    y, z = y * y_scale, z * y_scale
    stiff = st if stiff is None else stiff
    shape = tuple(y.shape)

    def score(x, t, yy):
        return -(x - yy) * stiff / (sde._std(t)[:, None, None, None] ** 2 + 0.1)

    def rhs(dtype):
        """the right-hand side of test_ode_controller_vs_solve_ivp (dtype complex64), or the same expression in complex128"""
        yy = y.to(dtype)
        real = torch.float32 if dtype == torch.complex64 else torch.float64

        def f(t, xf):
            x = torch.from_numpy(xf.reshape(shape)).to(dtype)
            vt = torch.ones(shape[0], dtype=real) * t
            gg = sde.diffusion(vt)[:, None, None, None]
            return (sde.theta * (yy - x) + (-(gg ** 2) * score(x, vt, yy) * 0.5)).numpy().reshape(-1)
        return f
    return sde, y, z, eps, score, rhs, shape


def _dist(a, b, zero_ref):
    return float(np.linalg.norm(a - b)) if zero_ref else float(np.linalg.norm(a - b) / np.linalg.norm(b))


# DOP853's case (a), the start state of exactly zero, on another y.  With _ivp_case's y (|y| ~ 0.3) scipy's own DOP853 needs 110 / 74
# evaluations (complex64 / complex128 right-hand side) at 1e-5, 86 / 62 at 1e-4 and 1e-3, and 206 / 158, 374 / 350 with the score times
# 40, 160: the first steps (h = 1e-6, 1e-5, ...) have no truncation error to speak of, so the estimate is the fp32 rounding of the
# right-hand side, about 6e-8 |f| h / atol, and scipy grows the step ten-fold only below (0.9 / 10)^8 = 4.3e-9 - with |f| ~ |y| ~ 0.3
# the rounding sits above that and picks every factor.  It is proportional to |y|: with y times 1e-3 (|y| ~ 3e-4, still 30 atol) the
# first steps grow by 10.0, 7.5, 4.9, 6.8 (the last three from the norm of the two sums and the exponent -1/8), and with the score times
# 40 the later ones are set by the truncation error (factors 1.0 ... 2.4).  scipy alone: 122 / 122 evaluations for each of the seeds 3 ...
# 8, 2.2e-5 from the 1e-12 solution.  RK23 keeps _ivp_case's (a) as it is.
ZERO_START = {"RK23": ("a", None, 1.0), "DOP853": ("a", 40.0, 1e-3)}          # (case of _ivp_case, score multiplier, y times)
CONTROLLER_CASES = [(m, c) for m in METHODS for c in ("a", "b", "c", "e", "rejections")]


@pytest.mark.parametrize("method,case", CONTROLLER_CASES)
def test_ode_controller_vs_solve_ivp(dev, method, case):
    """get_ode_sampler(method=M, denoise=False) against scipy.integrate.solve_ivp(method=M) with the right-hand side of
    tests/test_ode_kernels.py: (a) zero start state (DOP853: on y times 1e-3 with the score times 40, see ZERO_START), (b) everything zero (compared absolutely), (c) eps = 0.999: one clipped step, nfev =
    2 + n_stages, (e) three coupled rows, all at rtol = atol = 1e-5; and one case with rejected steps per method (RK23: the score times 40
    at 1e-5; DOP853: the score times 160 at 1e-3).  Before the engine runs the case is shown to be a fair one with scipy alone: the same
    nfev with the right-hand side in complex64 and in complex128, and an end state within 2.5e-4 of a DOP853 run at 1e-12 (so two valid
    runs differ by less than 5e-4).  Simulator (the same torch CPU right-hand side): nfev and nfev_rows equal, rel-L2 < 1e-7 (one
    complex64 rounding of the returned state).  Device: nfev within ONE attempted step (n_stages evaluations), rel-L2 < 1e-3."""
    from scipy.integrate import solve_ivp

    from storm_amd.sampling import get_ode_sampler
    tb = tableau(method)
    name, stiff, tol = REJECTION[method] if case == "rejections" else (case, None, 1e-5)
    y_scale = 1.0
    if case == "a":
        name, stiff, y_scale = ZERO_START[method]
    sde, y, z, eps, score, rhs, shape = _toy_problem(name, stiff, y_scale)
    z0 = z.numpy().reshape(-1)
    sol = solve_ivp(rhs(torch.complex64), (sde.T, eps), z0, rtol=tol, atol=tol, method=method)
    sol64 = solve_ivp(rhs(torch.complex128), (sde.T, eps), z0.astype(np.complex128), rtol=tol, atol=tol, method=method)
    exact = solve_ivp(rhs(torch.complex128), (sde.T, eps), z0.astype(np.complex128), rtol=1e-12, atol=1e-12, method="DOP853")
    assert sol.status == 0 and sol64.status == 0 and exact.status == 0
    zero_ref = case == "b"
    off = _dist(sol.y[:, -1], exact.y[:, -1], zero_ref)
    attempted, accepted = (sol.nfev - 2) // tb.n_stages, len(sol.t) - 1
    print(f"ode controller {method} ({case}): scipy nfev {sol.nfev} (complex128 right-hand side: {sol64.nfev}), {attempted - accepted} rejections, "
          f"{'abs' if zero_ref else 'rel'}-L2 from the 1e-12 solution {off:.3e}")
    assert sol.nfev == sol64.nfev                                         # the case does not hinge on the rounding of the right-hand side
    if case == "a":
        assert not z.any() and y.any()                                    # d0 = 0: h0 = 1e-6
    assert off < 2.5e-4
    assert (sol.nfev - 2) % tb.n_stages == 0
    if case == "c":
        assert sol.nfev == 2 + tb.n_stages == {"RK23": 5, "DOP853": 14}[method]
    if case == "rejections":
        assert attempted > accepted
    want = torch.from_numpy(sol.y[:, -1].reshape(shape))
    yd, zd = y.to(dev), z.to(dev)
    sampler = get_ode_sampler(sde, score, y=yd, eps=eps, noise_fn=lambda: zd, denoise=False, method=method, rtol=tol, atol=tol)
    x, nfe = sampler(z=zd)
    assert torch.equal(zd.cpu(), z)
    err = _dist(x.cpu().to(torch.complex128).numpy().reshape(-1), sol.y[:, -1], zero_ref)
    print(f"ode controller {method} ({case}): nfev {nfe} (scipy {sol.nfev}), {'abs' if zero_ref else 'rel'}-L2 vs solve_ivp {err:.3e}")
    assert want.shape == x.shape
    if dev.type == "cpu":
        assert nfe == sol.nfev and sampler.nfev_rows == [sol.nfev] * shape[0]
        assert err < 1e-7
    else:
        assert abs(nfe - sol.nfev) <= tb.n_stages
        assert err < 1e-3


# ---------------------------------------------------------------- 5. rows ------------------------------------------------
ROWS_SCORE = {"RK23": 1.0, "DOP853": 40.0}       # (DOP853 needs 38 evaluations for each of the three rows as they are: the score times 40 sets them apart)


@pytest.mark.parametrize("method", METHODS)
def test_ode_per_row_control(dev, method):
    """three rows of different scale with one step controller each: every row is bit-equal to its batch-1 run and needs its own number
    of evaluations; compact=True (finished rows leave) is bit-equal to compact=False, and evaluates fewer rows"""
    from storm_amd.sampling import get_ode_sampler
    sde, y, z, eps, score, _, shape = _toy_problem("e", ROWS_SCORE[method])
    yd, zd = y.to(dev), z.to(dev)
    kw = dict(eps=eps, denoise=False, method=method, rtol=1e-5, atol=1e-5, per_row=True)
    sampler = get_ode_sampler(sde, score, y=yd, noise_fn=lambda: zd, **kw)
    x, nfe = sampler()
    rows, evaluated = list(sampler.nfev_rows), sampler.rows_evaluated
    assert nfe == max(rows) and all((r - 2) % tableau(method).n_stages == 0 for r in rows)
    for b in range(shape[0]):
        alone = get_ode_sampler(sde, score, y=yd[b:b + 1], noise_fn=lambda: zd[b:b + 1], **kw)
        xb, nb = alone()
        assert bits_equal(xb, x[b:b + 1]) and [nb] == alone.nfev_rows == rows[b:b + 1], (b, nb, rows)
    idle = get_ode_sampler(sde, score, y=yd, noise_fn=lambda: zd, compact=False, **kw)
    xi, ni = idle()
    assert bits_equal(xi, x) and ni == nfe and idle.nfev_rows == rows
    assert idle.rows_evaluated == shape[0] * nfe
    print(f"ode rows {method}: nfev per row {rows}; rows evaluated {evaluated} (compact) / {idle.rows_evaluated}")
    assert len(set(rows)) > 1                                             # the rows finish apart ...
    assert evaluated == sum(rows) < shape[0] * nfe                        # ... and a finished row is not evaluated again


# ---------------------------------------------------------------- 6. fixture F25: the reference's own runs -----------------
@pytest.mark.parametrize("method,tol", OC.CASES)
def test_ode_methods_vs_reference(dev, golden, method, tol):
    """the reference's get_ode_sampler(method=M, rtol = atol = tol) on F7's problem, one utterance per call (fixture F25: kept only where the
    reference needs the same nfev with the score in complex64 and in complex128).  Simulator: nfev equal; device: within one attempted
    step; rel-L2 < 1e-3, the bound of the F7 test (test_sampler.py test_ode_sampler_vs_reference) on both."""
    from storm_amd.sampling import get_ode_sampler
    from storm_amd.sdes import OUVESDE
    g = golden["f25_ode_methods"]
    y, z = OC.inputs()
    assert str(g["input_hash"]) == OC.input_hash(y, z) and int(g["seed"]) == OC.SEED
    assert list(g[f"tried_{method}_{tol:g}_nfev32"]) == list(g[f"tried_{method}_{tol:g}_nfev64"])
    sde = OUVESDE(**OC.SDE)
    for b in range(y.shape[0]):
        zb = z[b:b + 1].to(dev)
        sampler = get_ode_sampler(sde, OC.make_score(sde), y=y[b:b + 1].to(dev), eps=OC.EPS, noise_fn=lambda: zb, method=method, rtol=tol, atol=tol)
        x, nfe = sampler()
        want = int(g[OC.key(method, tol, b) + "_nfev"])
        err = rel_l2(x.cpu(), g[OC.key(method, tol, b) + "_out"])
        print(f"F25 {method} rtol = atol = {tol:g}, utterance {b}: nfev {nfe} (reference {want}), rel-L2 vs reference {err:.3e}")
        assert nfe == want if dev.type == "cpu" else abs(nfe - want) <= tableau(method).n_stages
        assert err < 1e-3


# ---------------------------------------------------------------- 7. the surface ------------------------------------------
MODEL_KW = dict(sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5, nf=8)


def _score_model(dev):
    from oracle import ncsnpp_ref as NR
    from storm_amd.model import ScoreModel
    m = ScoreModel(backbone="ncsnpp", **dict(MODEL_KW))
    m.dnn.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=5))
    m.eval(no_ema=True)
    return m.to(dev)


def test_other_methods_are_refused_by_name(dev):
    """solve_ivp's implicit methods and solver classes are not built: NotImplementedError naming what was asked for, before anything runs"""
    from scipy.integrate import RK45

    from storm_amd.sampling import get_ode_sampler
    from storm_amd.sdes import OUVESDE
    sde = OUVESDE(1.5, 0.05, 0.5, N=30)
    y = torch.zeros(1, 1, 8, 16, dtype=torch.complex64, device=dev)
    for method in ("Radau", "BDF", "LSODA"):
        with pytest.raises(NotImplementedError, match=method):
            get_ode_sampler(sde, None, y=y, method=method)
    with pytest.raises(NotImplementedError, match="RK45"):
        get_ode_sampler(sde, None, y=y, method=RK45)
    m = _score_model(dev)
    with pytest.raises(NotImplementedError, match="Radau"):
        m.enhance(0.1 * torch.ones(1, 4000).to(dev), sampler_type="ode", method="Radau")


@pytest.mark.gpu
def test_enhance_with_rk23_equals_enhance_batch():
    """(On the device only: measured on the host simulator, RK23 at rtol = atol = 0.5 needs 14 evaluations of this network per run and
    an evaluation of a 256-bin spectrogram takes 6 s there - 190 s for this test; test_method_reaches_every_sampler is the simulator's
    share.)  ScoreModel.enhance(sampler_type="ode", method="RK23") runs RK23 (2 + 3 k evaluations; another result than RK45's) and
    equals enhance_batch of the same input"""
    from tests.backend import setup_backend
    dev = setup_backend("hip")
    m = _score_model(dev)
    tol = 2e-3
    y = (0.1 * torch.randn(1, 4500, generator=torch.Generator().manual_seed(17))).to(dev)
    kw = dict(sampler_type="ode", rtol=tol, atol=tol, seed=5)
    a = m.enhance(y, method="RK23", **kw)
    rows = list(m.last_nfev_rows)
    b, nfe = m.enhance_batch(y, method="RK23", return_nfe=True, **kw)
    assert a.shape == (4500,) and torch.isfinite(a).all() and torch.equal(a, b.cpu()[0])
    assert rows == [nfe] and (nfe - 2) % 3 == 0
    c = m.enhance(y, **kw)                                               # RK45, the default
    assert (m.last_nfev_rows[0] - 2) % 6 == 0 and not torch.equal(a, c)
    print(f"enhance: RK23 {nfe} evaluations, RK45 {m.last_nfev_rows[0]}")


def test_method_reaches_every_sampler(dev, monkeypatch):
    """No network evaluation: sampling.get_ode_sampler is replaced by a recorder that checks its arguments as the real one does and
    returns the start spectrogram.  method= must arrive there from enhance, from enhance_batch, from get_ode_sampler's per-utterance
    form (whose _slice_keys cuts row_seeds and must keep the rest) and from every micro-batch of a grouped enhance_stream"""
    from storm_amd import model as M
    from storm_amd.sampling import ode
    m = _score_model(dev)
    seen = []

    def recorder(sde, score_fn, y, **kw):
        real = ode.get_ode_sampler(sde, score_fn, y=y, **kw)             # (refuses what the real one refuses; evaluates nothing)
        seen.append((kw.get("method"), kw.get("rtol"), None if kw.get("row_seeds") is None else list(kw["row_seeds"]), y.shape[0]))

        def sampler():
            sampler.nfev_rows = [2] * y.shape[0]
            return y.clone(), 2
        assert callable(real)
        return sampler
    monkeypatch.setattr(M.sampling, "get_ode_sampler", recorder)
    y = (0.1 * torch.randn(2, 4500, generator=torch.Generator().manual_seed(17))).to(dev)
    m.enhance(y[:1], sampler_type="ode", method="RK23", rtol=0.25)
    m.enhance_batch(y, sampler_type="ode", method="DOP853", rtol=0.125)
    assert seen == [("RK23", 0.25, None, 1), ("DOP853", 0.125, None, 2)]
    del seen[:]
    Y = m._prepare(y)[0]
    m.get_ode_sampler(Y, minibatch=1, method="DOP853", rtol=0.5, row_seeds=[11, 12])()
    assert seen == [("DOP853", 0.5, [11], 1), ("DOP853", 0.5, [12], 1)]
    del seen[:]
    batches = [(y, None), (y[:1, :4000], None)]
    outs = m.enhance_stream(batches, sampler_type="ode", method="DOP853", rtol=0.5, seeds=[40, 41])
    assert sorted(seen, key=lambda r: -r[3]) == [("DOP853", 0.5, None, 2), ("DOP853", 0.5, None, 1)] and m.last_nfev_stream == [2, 2]
    assert [tuple(o.shape) for o in outs] == [(2, 4500), (1, 4000)]
    with pytest.raises(NotImplementedError, match="BDF"):
        m.enhance_stream(batches, sampler_type="ode", method="BDF")


@pytest.mark.gpu
def test_enhance_stream_with_dop853_equals_its_micro_batches_own_runs():
    """(On the device only: DOP853 needs 2 + 12 k evaluations of every micro-batch, twice, and the simulator walks every lane of a
    256-bin network - minutes; on the simulator test_method_reaches_every_sampler shows that the stream hands method= on.)
    enhance_stream over two micro-batches of different frame buckets hands method= to every micro-batch's sampler: each returns what
    its own enhance_batch(method="DOP853") returns, bit for bit, after 2 + 12 k evaluations"""
    from tests.backend import setup_backend
    dev = setup_backend("hip")
    m = _score_model(dev)
    g = torch.Generator().manual_seed(32)
    lens, tol = [[5003, 4500], [9000]], 2e-3
    batches = []
    for bl in lens:
        y = torch.zeros(len(bl), max(bl))
        for k, n in enumerate(bl):
            y[k, :n] = 0.1 * torch.randn(n, generator=g)
        batches.append((y.to(dev), bl if len(set(bl)) > 1 else None))
    kw = dict(sampler_type="ode", method="DOP853", rtol=tol, atol=tol)
    own, own_nfe = [], []
    for p, (yb, bl) in enumerate(batches):
        o, n = m.enhance_batch(yb, lengths=bl, seed=40 + p, return_nfe=True, **kw)
        assert all((r - 2) % 12 == 0 for r in m.last_nfev_rows) and n == max(m.last_nfev_rows)
        own.append(o)
        own_nfe.append(n)
    outs = m.enhance_stream(batches, seeds=[40, 41], **kw)
    assert m.last_nfev_stream == own_nfe
    for p in range(len(lens)):
        assert torch.equal(outs[p], own[p]), p
    print(f"enhance_stream DOP853: evaluations per micro-batch {own_nfe}")


@pytest.mark.gpu
def test_enhancement_cli_ode_method(tmp_path):
    """enhancement.py --sampler ode --ode-method RK23 --ode-rtol 0.03 --ode-atol 0.03 on two short files: the enhanced files equal
    enhance_batch(method="RK23", rtol=0.03, atol=0.03) of the same files; the flags are refused without --sampler ode"""
    from scipy.io import wavfile

    from oracle import ncsnpp_ref as NR
    from storm_amd import distributed as D
    from storm_amd.model import ScoreModel
    path = os.path.join(tmp_path, "score.ckpt")
    sd = NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=5)
    torch.save({"state_dict": {"dnn." + k: v for k, v in sd.items()}, "hyper_parameters": dict(backbone="ncsnpp", **MODEL_KW)}, path)
    noisy, out = os.path.join(tmp_path, "noisy"), os.path.join(tmp_path, "enhanced")
    os.makedirs(noisy)
    g = torch.Generator().manual_seed(9)
    wavs = [0.1 * torch.randn(n, generator=g) for n in (6000, 4321)]
    for i, w in enumerate(wavs):
        wavfile.write(os.path.join(noisy, f"u{i}.wav"), 16000, w.numpy().astype(np.float32))
    env = {k: v for k, v in dict(os.environ, PYTHONPATH=ROOT).items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    base = [sys.executable, os.path.join(ROOT, "enhancement.py"), "--test_dir", noisy, "--enhanced_dir", out, "--ckpt", path, "--mode", "score-only"]
    flags = ["--ode-method", "RK23", "--ode-rtol", "0.03", "--ode-atol", "0.03"]
    r = subprocess.run(base + ["--sampler", "ode", "--seed", "321"] + flags, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (no 'ema' entry in this checkpoint)
        m = ScoreModel.load_from_checkpoint(path, base_dir="", batch_size=1, num_workers=0, kwargs=dict(gpu=False))
    m.eval(no_ema=False)
    m = m.cuda()
    lens = [len(w) for w in wavs]
    buckets = D.bucket_by_frames(lens, 16)
    assert len(buckets) == 1                                             # one 64-frame bucket: one enhance_batch call of the CLI's
    ids = buckets[0]
    yb = torch.zeros(len(ids), max(lens))
    for k, i in enumerate(ids):
        yb[k, :lens[i]] = wavs[i]
    want, nfe = m.enhance_batch(yb, sampler_type="ode", N=50, method="RK23", rtol=0.03, atol=0.03, seed=321 + ids[0], lengths=[lens[i] for i in ids],
                                return_nfe=True)
    assert (nfe - 2) % 3 == 0
    for k, i in enumerate(ids):
        sr, x = wavfile.read(os.path.join(out, f"u{i}.wav"))
        assert sr == 16000 and x.shape == (lens[i],) and np.isfinite(x).all()
        w = want[k, :lens[i]].cpu()
        assert float(w.abs().max()) > 0 and rel_l2(torch.from_numpy(x), w) < 1e-6, i
    r = subprocess.run(base + flags[:2], env=env, capture_output=True, text=True, timeout=300)       # (argument parsing only: no device is opened)
    assert r.returncode != 0 and "only with --sampler ode" in r.stderr


# ---------------------------------------------------------------- 8. refusals of the new entry points (no kernel runs) -----
def test_wide_entry_points_refuse_bad_arguments(dev):
    from storm_amd import _lib as L
    from storm_amd import ops
    lib = L.lib()
    n = 4
    x = torch.zeros(2, n, dtype=torch.complex128, device=dev)
    o64, o32 = torch.zeros_like(x), torch.zeros(2, n, dtype=torch.complex64, device=dev)
    K = [torch.zeros(2, n, dtype=torch.complex64, device=dev) for _ in range(14)]
    out, scratch = torch.zeros(2 * 129, dtype=torch.float64, device=dev), torch.zeros(2 * 129 * 256, dtype=torch.float64, device=dev)
    cd = (C.c_double * 14)(*[0.5] * 14)
    hd = (C.c_double * 129)(*[-0.01] * 129)
    r, p = ops._r, L.ptr

    def refused(rc, text):
        msg = lib.storm_last_error().decode()
        assert rc != 0 and text in msg, (rc, msg)

    def combine(nt, B, Kp=None):
        return lib.storm_rk_combine_rows_wide(p(r(o64)), p(r(o32)), p(r(x)), Kp or ops._kptrs(K[:max(nt, 1)]), cd, nt, hd, B, n, L.stream())

    def pair(nt, B, scratch_len, Kp=None, h=hd):
        return lib.storm_rk_error_pair_rows(p(out), p(scratch), scratch_len, p(r(x)), None, Kp or ops._kptrs(K[:max(nt, 1)]), cd, cd, nt, h,
                                            ATOL, RTOL, B, n, L.stream())
    for nt in (0, 14, -1):
        refused(combine(nt, 2), "n_terms=%d outside 1..13" % nt)
        refused(pair(nt, 2, scratch.numel()), "n_terms=%d outside 1..13" % nt)
    for B in (0, 129):
        refused(combine(2, B), "B=%d outside 1..128" % B)
        refused(pair(2, B, scratch.numel()), "B=%d outside 1..128" % B)
    null_stage = (C.c_void_p * 13)(*([p(r(K[0]))] * 11 + [None, p(r(K[0]))]))
    refused(combine(13, 2, null_stage), "null stage 11")
    refused(pair(13, 2, scratch.numel(), null_stage), "null stage 11")
    # a scratch shorter than 2 sums x blocks x B (n = 4: one block per row)
    refused(pair(2, 2, 3), "scratch of 3 doubles < 4")
    assert pair(2, 2, 4) == 0 and pair(13, 2, 4, h=None) == 0 and combine(13, 2) == 0
    refused(lib.storm_rk_combine_rows_wide(None, None, p(r(x)), ops._kptrs(K[:2]), cd, 2, hd, 2, n, L.stream()), "storm_rk_combine_rows_wide: bad arguments")
    refused(lib.storm_rk_error_pair_rows(p(out), p(scratch), 4, p(r(x)), None, ops._kptrs(K[:2]), cd, None, 2, hd, ATOL, RTOL, 2, n, L.stream()),
            "null coefficients")
    with pytest.raises(ValueError):
        ops.rk_combine_rows_wide(x, [K[0]], [1.0], [-0.01])
    with pytest.raises(ValueError):
        ops.rk_error_pair_rows(x, None, [K[0]], [1.0], [1.0], [-0.01] * 3, ATOL, RTOL)
