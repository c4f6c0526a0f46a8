"""The probability-flow ODE solver's kernels and step controller, alone, against scipy's RK45.

storm_amd/sampling/ode.py re-implements scipy's RK45 on the device; its per-element algebra runs in rk_combine_rows_kernel,
rk_scaled_sumsq_rows_kernel + sum_rows_kernel and storm_copy_rows (storm_amd/csrc/sde.hip).  The sampler tests compare whole runs with
recorded end points at 1e-3; here every kernel is compared with a float64 / complex128 numpy restatement of the same expression at
the shapes where such kernels go wrong (less than a wave, one block + a partial one, the 128-row split of ops.py, the grid-stride
loops), under bounds DERIVED from the number formats.  The restatement itself is tied to scipy's own functions by one backend-free
test (the only one that touches scipy's private modules), and the controller is run against scipy.integrate.solve_ivp on cases the
recorded fixtures never reach.

Every tolerance is shown to be able to fail: next to a comparison the test evaluates the reference with one defect (a dropped
term, another row's step size, an unwritten tail, a missing block ...) in numpy and asserts that it lies more than 100 x the bound away.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch

from oracle import sde_ref as SR
from tests.backend import dev  # noqa: F401
from tests.util import rel_l2

ATOL = RTOL = 1e-5
U64, U32 = 2.0 ** -53, 2.0 ** -24            # unit roundoff of float64 / float32 (round to nearest)
BITES = 100.0                                # a defect must lie this many bounds away from the reference
GRID_CAP = 2048                              # sde.hip ew_blocks: blocks of 256 threads per row launch
ROW_BLOCKS = 256                             # STORM_RK_ROW_BLOCKS: blocks per row of the row reduction


# ---------------------------------------------------------------- the reference (numpy, float64 / complex128) ------------
def _col(h, like):
    h = np.asarray(h, dtype=np.float64)
    return h.reshape(h.shape + (1,) * (np.ndim(like) - h.ndim))


def _c128(a):
    return a.detach().cpu().numpy().astype(np.complex128) if torch.is_tensor(a) else np.asarray(a, dtype=np.complex128)


def ref_combine(x, K, c, h):
    """x + h * (K.T @ c): one Runge-Kutta stage (scipy's rk_step: y + h * np.dot(K[:s].T, a[:s])); h a scalar or one value per row"""
    return _c128(x) + _col(h, x) * np.tensordot(np.asarray(c, dtype=np.float64), np.stack([_c128(k) for k in K]), 1)


def ref_scaled_sumsq(v, ya, yb=None, atol=ATOL, rtol=RTOL):
    """sum |v|^2 / (atol + max(|ya|, |yb|) rtol)^2 over the last axis: scipy's norm(v / scale)^2 * size"""
    m = np.abs(ya) if yb is None else np.maximum(np.abs(ya), np.abs(yb))
    return (np.abs(v) ** 2 / (atol + m * rtol) ** 2).sum(-1)


def ref_initial_step(fun, t0, y0, f0, direction, order=4, atol=ATOL, rtol=RTOL, interval=np.inf):
    """scipy's select_initial_step from the scaled sums (the scalars ode.py forms on the host)"""
    n = y0.size
    d0, d1 = np.sqrt(ref_scaled_sumsq(y0, y0, None, atol, rtol) / n), np.sqrt(ref_scaled_sumsq(f0, y0, None, atol, rtol) / n)
    h0 = min(1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1, interval)
    f1 = fun(t0 + h0 * direction, y0 + h0 * direction * f0)
    d2 = np.sqrt(ref_scaled_sumsq(f1 - f0, y0, None, atol, rtol) / n) / h0
    h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1 / (order + 1))
    return min(100 * h0, h1, interval)


def _rv(a):
    """a complex array as its float components [..., 2] (the kernels round per component)"""
    a = np.asarray(a)
    return np.stack([a.real, a.imag], -1)


def magnitude(x, K, c, h):
    """|x| + |h| sum |c_j| |K_j| per float component: what one rounding of the combination is relative to"""
    return np.abs(_rv(_c128(x))) + np.abs(_col(h, x))[..., None] * sum(abs(float(cj)) * np.abs(_rv(_c128(k))) for cj, k in zip(c, K))


def bites(ref, defect, bound, what):
    """the comparison |got - ref| <= bound can fail: `defect` (the reference with one fault) lies > 100 bounds away somewhere"""
    d = np.abs(np.asarray(defect, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        far = np.nanmax(np.where(np.asarray(bound) > 0, d / bound, np.where(d > 0, np.inf, 0.0)))
    assert far > BITES, (what, far)


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


# ---------------------------------------------------------------- coefficients and inputs ---------------------------------
_RND = [0.31, -0.57, 0.83, -0.29, 0.47, -0.91, 0.63]         # no zero: a kernel that skipped any K[j] would be seen


def dp_coef(nt):
    """the Dormand-Prince row with nt terms: A[nt] (stages 1..5), B (6), E (7).  B[1] = E[1] = 0, hence the second set"""
    from storm_amd.sampling.ode import _A, _B, _E
    return list(_A[nt]) if nt <= 5 else (list(_B) if nt == 6 else list(_E))


def rnd_coef(nt):
    return _RND[:nt]


COEF_SETS = [("dormand-prince", dp_coef), ("non-zero", rnd_coef)]


def _crandn(g, *shape, dtype=torch.complex64):
    return torch.view_as_complex(torch.randn(*shape, 2, generator=g, dtype=torch.float64)).to(dtype)


@functools.lru_cache(maxsize=None)
def rows_case(B, n):
    """(x complex128 [B, n], xb complex128 (|xb| > |x| in about half of the elements), 7 stages complex64, one negative step size per
    row with row 1 = 0 when there is one).  Shared by the tests of a shape; never written to."""
    g = torch.Generator().manual_seed(7000 + 131 * B + n)
    x, xb = _crandn(g, B, n, dtype=torch.complex128) * 1.3, _crandn(g, B, n, dtype=torch.complex128) * 1.3
    K = tuple(_crandn(g, B, n) for _ in range(7))
    h = [-0.003 * (1 + b % 7) - 1e-4 * b for b in range(B)]
    if B > 1:
        h[1] = 0.0
    frac = float((xb.abs() > x.abs()).double().mean())
    assert n * B < 64 or 0.4 < frac < 0.6, frac
    return x, xb, K, h


def flat_case(n, seed=0):
    """fp32 one-state inputs: x, xb complex64 [n], 7 stages.  Stage j is 2^j times a standard normal: fp32 resolves a dropped last
    term only if that term matters, and the last coefficients of the Dormand-Prince rows 4 and 5 are a fortieth of their largest."""
    g = torch.Generator().manual_seed(9000 + seed + n % 1000)
    return _crandn(g, n) * 1.3, _crandn(g, n) * 1.3, [_crandn(g, n) * 2.0 ** j for j in range(7)]


ROW_CASES = [(3, 5), (3, 259), (130, 3)]             # less than a wave; one block + a partial one; across the 128-row split of ops.py
LONG_ROW = (1, GRID_CAP * 256 + 7)                   # the row launch caps at 2048 blocks: 7 threads go round the stride loop
SUM_CASES = ROW_CASES + [(2, 65536 + 7)]             # the row reduction caps at 256 blocks: 7 threads go round ITS loop
FLAT_BIG = 2 * GRID_CAP * 256 + 6                    # stride loop of the float4 combine (n / 2 float4s) and of the fp32 sum's 2048 blocks


# ---------------------------------------------------------------- 1. the restatement is scipy's ---------------------------
def test_reference_restatement_is_scipys_rk45():
    """No backend: ref_combine / ref_scaled_sumsq / ref_initial_step give scipy's y_new, error_norm^2 * size and h_abs (1e-14: float64,
    the same operations in another order), and ode.py's tableau is scipy's, exactly."""
    import inspect

    from scipy.integrate._ivp.common import norm, select_initial_step
    from scipy.integrate._ivp.rk import RK45, rk_step

    from storm_amd.sampling import ode
    assert np.array_equal(np.array(ode._C), RK45.C) and np.array_equal(np.array(ode._B), RK45.B) and np.array_equal(np.array(ode._E), RK45.E)
    for s in range(1, 6):
        assert np.array_equal(np.array(ode._A[s]), RK45.A[s][:s]) and not RK45.A[s][s:].any()
    rng = np.random.default_rng(5)
    n = 37
    y0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    M = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(n) - 2.0 * np.eye(n)
    fun = lambda t, y: M @ y                                             # noqa: E731  (a linear right-hand side)
    t0, t_end, direction = 1.0, 0.03, -1.0
    solver = RK45(fun, t0, y0, t_end, rtol=RTOL, atol=ATOL)
    assert ode._ERR_EXP == solver.error_exponent and solver.error_estimator_order == 4
    f0 = fun(t0, y0)
    # the initial step
    args = (fun, t0, y0, t_end, np.inf, f0, direction, 4, RTOL, ATOL)
    if "t_bound" not in inspect.signature(select_initial_step).parameters:  # (scipy < 1.12: no interval clipping)
        args = (fun, t0, y0, f0, direction, 4, RTOL, ATOL)
    h_abs = select_initial_step(*args)
    assert h_abs == solver.h_abs
    mine = ref_initial_step(fun, t0, y0, f0, direction, interval=abs(t_end - t0))
    assert abs(mine - h_abs) <= 1e-14 * h_abs, (mine, h_abs)
    assert abs(np.sqrt(ref_scaled_sumsq(f0, y0) / n) - norm(f0 / (ATOL + np.abs(y0) * RTOL))) <= 1e-14 * norm(f0 / (ATOL + np.abs(y0) * RTOL))
    # one step: y_new and the error norm
    h = -h_abs
    y_new, f_new = rk_step(fun, t0, y0, f0, h, RK45.A, RK45.B, RK45.C, solver.K)
    K = [solver.K[j] for j in range(7)]
    got = ref_combine(y0, K[:6], ode._B, h)
    mag = magnitude(y0, K[:6], ode._B, h)
    assert (np.abs(_rv(got) - _rv(y_new)) <= 1e-14 * mag).all()
    for s in range(1, 6):                                                # (the stages: K[s] = fun(t + c h, y + h K[:s].T @ a[:s]))
        ys = ref_combine(y0, K[:s], ode._A[s], h)
        assert np.abs(fun(t0 + ode._C[s] * h, ys) - K[s]).max() <= 1e-13 * np.abs(K[s]).max()
    scale = ATOL + np.maximum(np.abs(y0), np.abs(y_new)) * RTOL
    want = solver._estimate_error_norm(solver.K, h, scale) ** 2 * n
    mine = ref_scaled_sumsq(_col(h, y0) * np.tensordot(np.array(ode._E), np.stack(K), 1), y0, y_new)
    assert abs(mine - want) <= 1e-14 * want, (mine, want)


# ---------------------------------------------------------------- 2. rk_combine_rows --------------------------------------
def _combine_defects(x, K, c, h, ref, bound):
    nt = len(K)
    bites(_rv(ref), _rv(ref_combine(x, K[:nt - 1], c[:nt - 1], h) if nt > 1 else _c128(x) + 0 * ref), bound, "last term dropped")
    if len(h) > 1:
        bites(_rv(ref), _rv(ref_combine(x, K, c, [h[0]] * len(h))), bound, "row 0's h for every row")
    unwritten = ref.copy()
    unwritten.reshape(-1)[-7:] = 0
    bites(_rv(ref), _rv(unwritten), bound, "last 7 elements unwritten")


def _check_combine(dev, x, K, h, nt, coef, want_rows=False):
    """one (n_terms, coefficient set) of a shape: both want64 forms against the reference; returns the worst error in bounds"""
    from storm_amd import ops
    xd, Kd = x.to(dev), [k.to(dev) for k in K[:nt]]
    c = coef(nt)
    o64, o32 = ops.rk_combine_rows(xd, Kd, c, h, want64=True)
    only32 = ops.rk_combine_rows(xd, Kd, c, h)
    ref = ref_combine(x, K[:nt], c, h)
    # one rounding per fma on either side: the kernel's nt fma for the sum and one for x + h sum, as many for the reference
    bound = 2 * (nt + 1) * U64 * magnitude(x, K[:nt], c, h)
    err = np.abs(_rv(_c128(o64)) - _rv(ref))
    assert (err <= bound).all(), float((err / bound).max())
    _combine_defects(x, K[:nt], c, h, ref, bound)
    assert bits_equal(o32, o64.to(torch.complex64))                      # both round to nearest even
    assert bits_equal(only32, o32)
    for b, hb in enumerate(h):
        if hb == 0:
            assert bits_equal(o64[b], x[b])
    if want_rows:
        for b in range(x.shape[0]):
            a64, a32 = ops.rk_combine_rows(xd[b:b + 1], [k[b:b + 1] for k in Kd], c, h[b:b + 1], want64=True)
            assert bits_equal(a64, o64[b:b + 1]) and bits_equal(a32, o32[b:b + 1]), b
    return float((err / bound).max())


@pytest.mark.parametrize("B,n", ROW_CASES)
def test_rk_combine_rows_vs_reference(dev, B, n):
    """out64 within 2 (n_terms + 1) 2^-53 (|x| + |h| sum |c_j| |K_j|) per component, out32 its rounding, the h = 0 row untouched, every
    row bit-equal to its own B = 1 call; n_terms 1..7 with the Dormand-Prince rows and with non-zero coefficients"""
    x, _, K, h = rows_case(B, n)
    assert 0.0 in h and all(v <= 0 for v in h) and len(set(h)) > 2
    worst = 0.0
    for name, coef in COEF_SETS:
        for nt in range(1, 8):
            worst = max(worst, _check_combine(dev, x, K, h, nt, coef, want_rows=(nt == 7)))
    print(f"rk_combine_rows [{B}, {n}]: worst error {worst:.3g} of the bound (bound = 2 (n_terms + 1) 2^-53 magnitude)")


def test_rk_combine_rows_stride_loop(dev):
    """a row of 2048 * 256 + 7 elements: the last 7 are written in the grid-stride loop's second round (n_terms = 2 keeps it small)"""
    B, n = LONG_ROW
    g = torch.Generator().manual_seed(77)
    x, K, h = _crandn(g, B, n, dtype=torch.complex128) * 1.3, [_crandn(g, B, n) for _ in range(2)], [-0.0137]
    worst = _check_combine(dev, x, K, h, 2, rnd_coef)
    print(f"rk_combine_rows [{B}, {n}]: worst error {worst:.3g} of the bound")


# ---------------------------------------------------------------- 3. rk_scaled_sumsq_rows ---------------------------------
def _last_block_missing(terms, n):
    """the row sum without the share of the row's last block (block of element i: (i / 256) mod blocks)"""
    nb = min((n + 255) // 256, ROW_BLOCKS)
    keep = (np.arange(n) // 256) % nb != nb - 1
    return (terms * keep).sum(-1)


def _sum_terms(v, ya, yb):
    m = np.abs(ya) if yb is None else np.maximum(np.abs(ya), np.abs(yb))
    return np.abs(v) ** 2 / (ATOL + m * RTOL) ** 2


def _check_sums(got, ref, n, what):
    """rows whose reference is zero are exactly zero; the others within (n + 64) 2^-53 of it: n roundings of the summation in any
    order (all terms positive) and a few dozen per term; returns the worst error in bounds"""
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float64 and got.shape == ref.shape
    bound = (n + 64) * U64 * ref
    err = np.abs(got - ref)
    assert (got[ref == 0] == 0.0).all(), what
    assert (err <= bound).all(), (what, got, ref)
    return float((err[ref > 0] / bound[ref > 0]).max()) if (ref > 0).any() else 0.0


@pytest.mark.parametrize("B,n", SUM_CASES)
def test_rk_scaled_sumsq_rows_vs_reference(dev, B, n):
    """the embedded-error form (n_terms 1..7, both coefficient sets, xb given, per-row h with one 0) and the three initial-step forms
    (xb = None, h_rows = None) against the reference sum; every row bit-equal to its B = 1 call"""
    from storm_amd import ops
    x, xb, K, h = rows_case(B, n)
    xn, xbn, Kn = _c128(x), _c128(xb), [_c128(k) for k in K]
    xd, xbd, Kd = x.to(dev), xb.to(dev), [k.to(dev) for k in K]
    worst = 0.0
    nz = [b for b, v in enumerate(h) if v != 0]

    def alone(b, K_, c, h_, mode, xb_):
        return ops.rk_scaled_sumsq_rows(xd[b:b + 1], None if xb_ is None else xb_[b:b + 1], [k[b:b + 1] for k in K_], c,
                                        None if h_ is None else h_[b:b + 1], ATOL, RTOL, mode=mode)

    for name, coef in COEF_SETS:
        for nt in range(1, 8):
            c = coef(nt)
            got = ops.rk_scaled_sumsq_rows(xd, xbd, Kd[:nt], c, h, ATOL, RTOL)
            v = _col(h, xn) * np.tensordot(np.array(c), np.stack(Kn[:nt]), 1)
            terms = _sum_terms(v, xn, xbn)
            ref = terms.sum(-1)
            assert (ref[[b for b, hv in enumerate(h) if hv == 0]] == 0).all() and (ref[nz] > 0).all()
            worst = max(worst, _check_sums(got, ref, n, (name, nt)))
            bound = (n + 64) * U64 * ref[nz]
            bites(ref[nz], _sum_terms(v, xn, None).sum(-1)[nz], bound, "|xa| alone in the scale")
            vd = _col(h, xn) * np.tensordot(np.array(c[:nt - 1]), np.stack(Kn[:nt - 1]), 1) if nt > 1 else 0 * v
            bites(ref[nz], _sum_terms(vd, xn, xbn).sum(-1)[nz], bound, "last term dropped")
            bites(ref[nz], _last_block_missing(terms, n)[nz], bound, "last block's share missing")
            if nt == 7:
                for b in range(B):
                    assert bits_equal(alone(b, Kd[:nt], c, h, None, xbd), got[b:b + 1]), (name, b)
    for mode, Km in ((-1, Kd[:1]), (-2, Kd[:2]), (-3, [])):
        got = ops.rk_scaled_sumsq_rows(xd, None, Km, None, None, ATOL, RTOL, mode=mode)
        v = {-1: Kn[0], -2: Kn[0] - Kn[1], -3: xn}[mode]
        terms = _sum_terms(v, xn, None)
        ref = terms.sum(-1)
        worst = max(worst, _check_sums(got, ref, n, mode))
        bound = (n + 64) * U64 * ref
        bites(ref, _last_block_missing(terms, n), bound, "last block's share missing")
        if mode == -2:
            bites(ref, _sum_terms(Kn[0], xn, None).sum(-1), bound, "last term dropped")
        for b in range(B):
            assert bits_equal(alone(b, Km, None, None, mode, None), got[b:b + 1]), (mode, b)
    print(f"rk_scaled_sumsq_rows [{B}, {n}]: worst error {worst:.3g} of the bound (bound = (n + 64) 2^-53 relative)")


def test_rk_scaled_sumsq_rows_scratch_grows_with_the_batch(dev):
    """ops.py caches the partial-sum scratch per host thread and grows it: on a thread of its own (so the cache starts empty) a call
    with B = 1, then B = 3, then B = 2 gives the right numbers each time"""
    from storm_amd import ops
    x, xb, K, h = rows_case(3, 259)
    xn, xbn, Kn = _c128(x), _c128(xb), [_c128(k) for k in K]
    xd, xbd, Kd = x.to(dev), xb.to(dev), [k.to(dev) for k in K]
    c = rnd_coef(7)
    ref = _sum_terms(_col(h, xn) * np.tensordot(np.array(c), np.stack(Kn), 1), xn, xbn).sum(-1)
    res = {}

    def run():
        try:
            key = (str(xd.device), threading.get_ident())
            ops._rk_scratch.pop(key, None)                               # (thread identifiers are reused: start without a buffer)
            for rows in (slice(0, 1), slice(0, 3), slice(1, 3)):
                res[rows.start, rows.stop] = ops.rk_scaled_sumsq_rows(xd[rows], xbd[rows], [k[rows] for k in Kd], c, h[rows], ATOL, RTOL).cpu()
            res["len"] = ops._rk_scratch[key].numel()
        except BaseException as e:                                       # (an exception on a thread is not the test's otherwise)
            res["error"] = e
        finally:
            ops._rk_scratch.pop((str(xd.device), threading.get_ident()), None)
    th = threading.Thread(target=run)
    th.start()
    th.join()
    assert "error" not in res, res["error"]
    assert res["len"] == 3 * ROW_BLOCKS
    for (a, b) in ((0, 1), (0, 3), (1, 3)):
        _check_sums(res[a, b], ref[a:b], 259, (a, b))


# ---------------------------------------------------------------- 4. copy_rows --------------------------------------------
def _masks(B):
    mid = [B // 3 <= b < max(B // 3 + 1, 2 * B // 3) for b in range(B)]
    return {"none": [False] * B, "all": [True] * B, "alternating": [b % 2 == 0 for b in range(B)], "one run in the middle": mid,
            "first row only": [b == 0 for b in range(B)], "last row only": [b == B - 1 for b in range(B)]}


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64, torch.float32])
def test_copy_rows(dev, dtype):
    """the selected rows are src's, every other row of dst is untouched, bit for bit"""
    from storm_amd import ops
    g = torch.Generator().manual_seed(44)
    for B, n in ((1, 3), (5, 3), (5, 259), (130, 3)):
        mk = (lambda: torch.randn(B, n, generator=g)) if dtype == torch.float32 else (lambda: _crandn(g, B, n, dtype=dtype))
        dst0, src = mk(), mk()
        for name, mask in _masks(B).items():
            dst = dst0.clone().to(dev)
            out = ops.copy_rows(dst, src.to(dev), mask)
            assert out is dst
            want = torch.where(torch.tensor(mask)[:, None], src, dst0)
            assert bits_equal(dst, want), (B, n, name)
            if any(mask) and not all(mask):
                assert not bits_equal(want, dst0) and not bits_equal(want, src)


# ---------------------------------------------------------------- 5. the exported entry points nothing else calls ----------
def _raw():
    from storm_amd import _lib as L
    from storm_amd import ops
    return L, L.lib(), ops


def _f32(v):
    return float(np.float32(v))


def _flat_refs(x, K, c, h):
    """float64 evaluation of the fp32 entry points' expression from the same fp32 inputs, coefficients and h rounded to fp32 first"""
    c32, h32 = [_f32(v) for v in c], _f32(h)
    return c32, h32, ref_combine(x, K, c32, h32), magnitude(x, K, c32, h32)


@pytest.mark.parametrize("n", [2, 258, FLAT_BIG])
def test_storm_rk_combine_fp32(dev, n):
    """storm_rk_combine (the one-state fp32 form, float4 per thread) within (n_terms + 1) 2^-24 (|x| + |h| sum |c_j| |K_j|) of the float64
    value of the same expression: one rounding per fmaf.  The largest size is the float4 form's stride loop."""
    L, lib, ops = _raw()
    x, _, K = flat_case(n)
    xd, Kd = x.to(dev), [k.to(dev) for k in K]
    h, worst = -0.037, 0.0
    for name, coef in COEF_SETS:
        for nt in (1, 4, 7):
            c = coef(nt)
            out = torch.empty_like(xd)
            L.check(lib.storm_rk_combine(L.ptr(ops._r(out)), L.ptr(ops._r(xd)), ops._kptrs(Kd[:nt]), (C.c_float * nt)(*c), nt, h, n, L.stream()),
                    "storm_rk_combine")
            c32, h32, ref, mag = _flat_refs(x, K[:nt], c, h)
            bound = (nt + 1) * U32 * mag
            err = np.abs(_rv(_c128(out)) - _rv(ref))
            assert (err <= bound).all(), (name, nt, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            bites(_rv(ref), _rv(ref_combine(x, K[:nt - 1], c32[:nt - 1], h32) if nt > 1 else _c128(x)), bound, "last term dropped")
            unwritten = ref.copy()
            unwritten[-7:] = 0
            bites(_rv(ref), _rv(unwritten), bound, "last elements unwritten")
    print(f"storm_rk_combine n = {n}: worst error {worst:.3g} of the bound (bound = (n_terms + 1) 2^-24 magnitude)")


def _flat_sumsq(L, lib, ops, dev, xd, xbd, Kd, c, n_terms, h, n, scratch_len):
    out = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
    scratch = torch.zeros(scratch_len, dtype=torch.float64, device=dev)
    nk = abs(n_terms)
    cf = (C.c_float * nk)(*c) if c is not None else None
    L.check(lib.storm_rk_scaled_sumsq(L.ptr(out), L.ptr(scratch), scratch_len, L.ptr(ops._r(xd)), L.ptr(ops._r(xbd)) if xbd is not None else None,
                                      ops._kptrs(Kd[:nk]), cf, n_terms, h, ATOL, RTOL, n, L.stream()), "storm_rk_scaled_sumsq")
    return float(out.cpu())


def _scale32(x, xb):
    m = np.abs(_c128(x)) if xb is None else np.maximum(np.abs(_c128(x)), np.abs(_c128(xb)))
    return _f32(ATOL) + m * _f32(RTOL)


@pytest.mark.parametrize("n", [2, 258, FLAT_BIG])
def test_storm_rk_scaled_sumsq_fp32(dev, n):
    """storm_rk_scaled_sumsq within 4 (n_terms + 4) 2^-24 A of the float64 value, A = sum (|h| sum |c_j| |K_j|)^2 / scale^2 (the sum without
    cancellation: it bounds the fp32 error of v even where the E coefficients cancel); with an ample scratch and with scratch_len = 3
    (the launch is capped to 3 blocks and strides).  The largest size reaches the stride loop of the 2048-block launch."""
    L, lib, ops = _raw()
    x, xb, K = flat_case(n, seed=1)
    if n == FLAT_BIG:
        # One block of 2048 holds 1 / 2048 of a uniform sum and the stride loop's third round 6 elements of a million: less than fp32
        # resolves.  The stages of the last block's elements are 30 x and those of the last 6 elements 300 x larger, so that either
        # share is a third of the sum and a sum without it is far outside the bound.
        w = torch.ones(n)
        w[(torch.arange(n) // 256) % GRID_CAP == GRID_CAP - 1] = 30.0
        w[-6:] = 300.0
        K = [k * w for k in K]
    xd, xbd, Kd = x.to(dev), xb.to(dev), [k.to(dev) for k in K]
    Kn = [_c128(k) for k in K]
    h, worst = -0.037, 0.0
    sets = COEF_SETS if n < FLAT_BIG else COEF_SETS[1:]                 # (the long case once: with the coefficients that hide no stage)
    sc = _scale32(x, xb)
    for name, coef in sets:
        for nt in range(1, 8):
            c = coef(nt)
            c32, h32 = [_f32(v) for v in c], _f32(h)
            v = h32 * np.tensordot(np.array(c32), np.stack(Kn[:nt]), 1)
            terms = np.abs(v) ** 2 / sc ** 2
            ref = terms.sum()
            A = ((abs(h32) * sum(abs(cj) * np.abs(k) for cj, k in zip(c32, Kn[:nt]))) ** 2 / sc ** 2).sum()
            bound = 4 * (nt + 4) * U32 * A
            for scratch_len in (4096, 3):
                got = _flat_sumsq(L, lib, ops, dev, xd, xbd, Kd, c, nt, h, n, scratch_len)
                assert abs(got - ref) <= bound, (name, nt, scratch_len, got, ref, abs(got - ref) / (U32 * A))
                worst = max(worst, abs(got - ref) / bound)
            bites(ref, (np.abs(v) ** 2 / _scale32(x, None) ** 2).sum(), bound, "|xa| alone in the scale")
            vd = h32 * np.tensordot(np.array(c32[:nt - 1]), np.stack(Kn[:nt - 1]), 1) if nt > 1 else 0 * v
            bites(ref, (np.abs(vd) ** 2 / sc ** 2).sum(), bound, "last term dropped")
            for nb in (min((n + 255) // 256, GRID_CAP), min((n + 255) // 256, 3)):
                bites(ref, (terms * ((np.arange(n) // 256) % nb != nb - 1)).sum(), bound, "last block's share missing")
            if n == FLAT_BIG:
                bites(ref, terms[:-6].sum(), bound, "the stride loop's last round missing")
    if n < FLAT_BIG:
        for mode in (-1, -2):
            for with_xb in (True, False):
                scm = _scale32(x, xb if with_xb else None)
                v = Kn[0] if mode == -1 else Kn[0] - Kn[1]
                ref = (np.abs(v) ** 2 / scm ** 2).sum()
                A = ((np.abs(Kn[0]) + (np.abs(Kn[1]) if mode == -2 else 0)) ** 2 / scm ** 2).sum()
                bound = 4 * (-mode + 4) * U32 * A
                for scratch_len in (4096, 3):
                    got = _flat_sumsq(L, lib, ops, dev, xd, xbd if with_xb else None, Kd, None, mode, 1.0, n, scratch_len)
                    assert abs(got - ref) <= bound, (mode, with_xb, scratch_len, got, ref)
                    worst = max(worst, abs(got - ref) / bound)
                if mode == -2:
                    bites(ref, (np.abs(Kn[0]) ** 2 / scm ** 2).sum(), bound, "last term dropped")
                if with_xb:
                    bites(ref, (np.abs(v) ** 2 / _scale32(x, None) ** 2).sum(), bound, "|xa| alone in the scale")
    print(f"storm_rk_scaled_sumsq n = {n}: worst error {worst:.3g} of the bound (bound = 4 (n_terms + 4) 2^-24 A)")


@pytest.mark.parametrize("n", [5, 259])
def test_storm_ouve_pf_drift_t_form(dev, n):
    """storm_ouve_pf_drift (g(t_b) formed in the kernel from t) against the oracle's probability-flow drift, at the step kernels' bound"""
    L, lib, ops = _raw()
    g = torch.Generator().manual_seed(9)
    x, y, s = [_crandn(g, 3, n) * 0.5 for _ in range(3)]
    t = torch.tensor([1.0, 0.5, 0.03])
    out = torch.empty_like(x, device=dev)
    xd, yd, sd, td = x.to(dev), y.to(dev), s.to(dev), t.to(dev)         # (held in locals: a temporary's memory is reused by the next one)
    L.check(lib.storm_ouve_pf_drift(L.ptr(ops._r(out)), L.ptr(ops._r(xd)), L.ptr(ops._r(yd)), L.ptr(ops._r(sd)), L.ptr(td), 3, n,
                                    L.Ouve(1.5, 0.05, 0.5, 30), L.stream()), "storm_ouve_pf_drift")
    sde = SR.OUVE(1.5, 0.05, 0.5, N=30)
    ref = SR.pf_drift(sde, lambda *_: s, x, t, y)
    err = rel_l2(out.cpu(), ref)
    print(f"storm_ouve_pf_drift [3, {n}]: rel-L2 vs oracle {err:.3e}")
    assert err < 3e-7
    assert rel_l2(SR.pf_drift(sde, lambda *_: s, x, t[:1].expand(3), y), ref) > BITES * 3e-7      # row 0's t for every row


# ---------------------------------------------------------------- 6. batch_l2norm -----------------------------------------
def test_batch_l2norm(dev):
    """fp64 accumulation, one rounding to fp32 (2^-24): within 2^-23 of the float64 norm of the fp32 data"""
    from storm_amd import ops
    g = torch.Generator().manual_seed(6)
    worst = 0.0
    for B, n in ((3, 1), (2, 127), (2, 129), (1, 1000)):
        v = _crandn(g, B, n)
        got = ops.batch_l2norm(v.to(dev)).cpu()
        assert got.dtype == torch.float32 and got.shape == (B,)
        fl = torch.view_as_real(v).double().flatten(1).numpy()
        ref = np.sqrt((fl ** 2).sum(1))
        err = np.abs(got.double().numpy() - ref) / ref
        assert (err <= 2 * U32).all(), (B, n, err)
        worst = max(worst, float(err.max() / (2 * U32)))
        bites(ref, np.sqrt((fl[:, :-1] ** 2).sum(1)), 2 * U32 * ref, "last float dropped")
        if B > 1:
            bites(ref, np.repeat(ref[:1], B), 2 * U32 * ref, "row 0 for every row")
    print(f"batch_l2norm: worst error {worst:.3g} of the bound (bound = 2^-23 relative)")


# ---------------------------------------------------------------- 7. the controller against scipy.integrate.solve_ivp --------
def _ivp_case(name):
    g = torch.Generator().manual_seed(3)
    y = _crandn(g, 1, 1, 8, 16) * 0.3
    z = y + 0.5 * _crandn(g, 1, 1, 8, 16)
    zero = torch.zeros_like(y)
    if name == "e":                                                      # three rows of different scale, ONE solver state over the batch
        g = torch.Generator().manual_seed(31)
        y = _crandn(g, 3, 1, 8, 16) * torch.tensor([0.1, 0.4, 1.5])[:, None, None, None]
        return y, y + 0.5 * _crandn(g, 3, 1, 8, 16), 0.03, 1.0
    return {"a": (y, zero, 0.03, 1.0), "b": (zero, zero, 0.03, 1.0), "c": (y, z, 0.999, 1.0), "d": (y, z, 0.03, 40.0)}[name]


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_ode_controller_vs_solve_ivp(dev, case):
    """get_ode_sampler(denoise=False) against scipy.integrate.solve_ivp(RK45, rtol = atol = 1e-5) over the flattened complex state with
    the same torch right-hand side on the CPU.  (a) the start state is exactly zero: d0 = 0, the first h0 = 1e-6 branch; (b) y and the
    start state both zero: the right-hand side vanishes, d1 = d2 = 0, which is also the only way into the h1 = max(1e-6, h0 * 1e-3)
    branch of the initial-step rule (compared absolutely: the reference is zero); (c) eps = 0.999: the
    first step is clipped to t_end, nfev = 8; (d) the score times 40: rejected steps; (e) the coupled form on three rows of different
    scale: the norms run over several rows.  On the host simulation the right-hand side is the same torch CPU arithmetic, so nfev is
    equal and the end point differs by the complex64 rounding of the returned state (one fp32 rounding = 6e-8: < 1e-7).  On the
    device an ulp in pow / div may move a step (as the F12 test records): nfev within 6, rel-L2 < 1e-3."""
    from scipy.integrate import solve_ivp

    from storm_amd.sampling import get_ode_sampler
    from storm_amd.sdes import OUVESDE
    sde = OUVESDE(1.5, 0.05, 0.5, N=30)
    y, z, eps, stiff = _ivp_case(case)
    shape = tuple(y.shape)

    def score(x, t, yy):
        return -(x - yy) * stiff / (sde._std(t)[:, None, None, None] ** 2 + 0.1)

    def rhs(t, xf):
        x = torch.from_numpy(xf.reshape(shape)).to(torch.complex64)
        vt = torch.ones(shape[0]) * t
        gg = sde.diffusion(vt)[:, None, None, None]
        return (sde.theta * (y - x) + (-(gg ** 2) * score(x, vt, y) * 0.5)).numpy().reshape(-1)
    sol = solve_ivp(rhs, (sde.T, eps), z.numpy().reshape(-1), rtol=RTOL, atol=ATOL, method="RK45")
    assert sol.status == 0
    want = torch.from_numpy(sol.y[:, -1].reshape(shape))
    yd, zd = y.to(dev), z.to(dev)
    sampler = get_ode_sampler(sde, score, y=yd, eps=eps, noise_fn=lambda: zd, denoise=False)
    x, nfe = sampler(z=zd)
    assert torch.equal(zd.cpu(), z)                                      # the caller's start state is not written to
    if case == "b":
        err = float((x.cpu().to(torch.complex128) - want).abs().pow(2).sum().sqrt())
        print(f"ode controller ({case}): nfev {nfe} (scipy {sol.nfev}), abs-L2 vs solve_ivp {err:.3e} [rel-L2 undefined: the reference is zero]")
    else:
        err = rel_l2(x.cpu(), want)
        print(f"ode controller ({case}): nfev {nfe} (scipy {sol.nfev}), rel-L2 vs solve_ivp {err:.3e}")
    if case == "c":
        assert sol.nfev == 8
    if case == "d":
        assert (sol.nfev - 2) // 6 > len(sol.t) - 1                      # more attempted steps than accepted ones: rejections
    if dev.type == "cpu":
        assert nfe == sol.nfev and sampler.nfev_rows == [sol.nfev] * shape[0]
        assert err < 1e-7
    else:
        assert abs(nfe - sol.nfev) <= 6
        assert err < 1e-3


# ---------------------------------------------------------------- 8. refusals (no kernel runs) ------------------------------
def test_solver_entry_points_refuse_bad_arguments(dev):
    L, lib, ops = _raw()
    n = 4
    x = torch.zeros(2, n, dtype=torch.complex128, device=dev)
    o64, o32 = torch.zeros_like(x), torch.zeros(2, n, dtype=torch.complex64, device=dev)
    K = [torch.zeros(2, n, dtype=torch.complex64, device=dev) for _ in range(8)]
    out, scratch = torch.zeros(129, dtype=torch.float64, device=dev), torch.zeros(129 * ROW_BLOCKS, dtype=torch.float64, device=dev)
    cd, cf = (C.c_double * 8)(*[0.5] * 8), (C.c_float * 8)(*[0.5] * 8)
    hd = (C.c_double * 129)(*[-0.01] * 129)
    r, p = ops._r, L.ptr

    def refused(rc, text):
        msg = lib.storm_last_error().decode()
        assert rc != 0 and text in msg, (rc, msg)

    def combine_rows(nt, B, Kp=None):
        return lib.storm_rk_combine_rows(p(r(o64)), p(r(o32)), p(r(x)), Kp or ops._kptrs(K[:max(nt, 1)]), cd, nt, hd, B, n, L.stream())

    def sumsq_rows(nt, B, scratch_len, Kp=None):
        return lib.storm_rk_scaled_sumsq_rows(p(out), p(scratch), scratch_len, p(r(x)), None, Kp or ops._kptrs(K[:max(nt, 1)]), cd, nt, hd,
                                              ATOL, RTOL, B, n, L.stream())
    refused(combine_rows(2, 129), "outside 1..128")
    refused(sumsq_rows(2, 129, scratch.numel()), "outside 1..128")
    refused(combine_rows(2, 0), "outside 1..128")
    for nt in (0, 8):
        refused(combine_rows(nt, 2), "storm_rk")
        refused(sumsq_rows(nt, 2, scratch.numel()), "n_terms=%d" % nt)
    refused(sumsq_rows(-4, 2, scratch.numel()), "n_terms=-4")
    # a rows scratch shorter than blocks x B (n = 4: one block per row)
    refused(sumsq_rows(2, 2, 1), "scratch of 1 doubles < 2")
    assert sumsq_rows(2, 2, 2) == 0
    null_stage = (C.c_void_p * 2)(p(r(K[0])), None)
    refused(combine_rows(2, 2, null_stage), "null stage 1")
    refused(sumsq_rows(2, 2, scratch.numel(), null_stage), "null stage 1")
    # the fp32 one-state forms
    xf, of = torch.zeros(n, dtype=torch.complex64, device=dev), torch.zeros(n + 1, dtype=torch.complex64, device=dev)
    Kf = [torch.zeros(n + 1, dtype=torch.complex64, device=dev) for _ in range(8)]

    def combine(nt, nc, Kp=None):
        return lib.storm_rk_combine(p(r(of)), p(r(xf)), Kp or ops._kptrs(Kf[:max(nt, 1)]), cf, nt, -0.01, nc, L.stream())

    def sumsq(nt, scratch_len, Kp=None):
        return lib.storm_rk_scaled_sumsq(p(out), p(scratch), scratch_len, p(r(xf)), None, Kp or ops._kptrs(Kf[:max(abs(nt), 1)]), cf, nt, -0.01,
                                         ATOL, RTOL, n, L.stream())
    refused(combine(2, 3), "storm_rk_combine: bad arguments")            # an odd n_complex (two complex per float4)
    assert combine(2, 4) == 0
    for nt in (0, 8):
        refused(combine(nt, 4), "storm_rk")
        refused(sumsq(nt, 16), "n_terms=%d" % nt)
    refused(sumsq(-3, 16), "n_terms=-3")                                 # (the state-itself form exists in the rows form only)
    refused(sumsq(2, 0), "storm_rk_scaled_sumsq: bad arguments")
    null_f = (C.c_void_p * 2)(p(r(Kf[0])), None)
    refused(combine(2, 4, null_f), "null stage 1")
    refused(sumsq(2, 16, null_f), "null stage 1")
    # through ops: per-row step sizes of the wrong length
    xs, Ks = x, [K[0]]
    with pytest.raises(ValueError):
        ops.rk_combine_rows(xs, Ks, [1.0], [-0.01])
    with pytest.raises(ValueError):
        ops.rk_combine_rows(xs, Ks, [1.0], [-0.01] * 3)
    with pytest.raises(ValueError):
        ops.rk_scaled_sumsq_rows(xs, None, Ks, [1.0], [-0.01], ATOL, RTOL)
