"""Fixture F25 (tests/golden/f25_ode_methods.npz): the cases and seeds shared by tools/make_golden_ode_methods.py and tests/test_ode_methods.py.

The reference hands `method` to scipy.integrate.solve_ivp (sampling/__init__.py:71-141).  F25 records its own get_ode_sampler runs with
method = RK23 and DOP853 on fixture F7's problem (oracle/make_golden.py gen_f7: the seeded [2, 1, 8, 16] state, the analytic score, OUVE
theta 1.5, sigma 0.05 .. 0.5, eps 0.03), one utterance per call as the reference model makes them (model.py:224-244, minibatch = 1).

A case is kept only where the run does not hinge on rounding: the generator runs every (method, tolerance) with the score evaluated in
complex64 and again in complex128 and keeps it if every utterance needs the same number of evaluations both times (DOP853's order-8 error
estimate can sit in the fp32 noise of the right-hand side at tight tolerances; a step sequence that depends on that noise cannot be
asked of another implementation).  TOLERANCES are tried in this order until CASES_PER_METHOD cases of a method are kept.
"""
import hashlib

import torch

SEED = 77
SHAPE = (2, 1, 8, 16)
SDE = dict(theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30)
EPS = 0.03
METHODS = ("RK23", "DOP853")
TOLERANCES = (1e-5, 1e-4, 1e-3)
CASES_PER_METHOD = 2

# what the generator's selection kept (it refuses to write a fixture that disagrees with this list)
CASES = [("RK23", 1e-5), ("RK23", 1e-4), ("DOP853", 1e-5), ("DOP853", 1e-3)]       # (DOP853 at 1e-4: 26 / 26 against 38 / 26 evaluations)


def inputs():
    """(y, z): gen_f7's draws - the noisy state and the prior noise, complex64 [2, 1, 8, 16]"""
    from oracle import sde_ref as SR
    g = torch.Generator().manual_seed(SEED)
    y = torch.randn(*SHAPE, dtype=torch.complex64, generator=g) * 0.3
    z = SR.complex_randn(y.shape, g)
    return y, z


def make_score(sde, double=False):
    """gen_f7's analytic score; double=True: the same expression evaluated in complex128 / float64 from the complex64 state"""
    def score(x, t, yy):
        if double:
            x, t, yy = x.to(torch.complex128), t.double(), yy.to(torch.complex128)
        return -(x - yy) / (sde._std(t)[:, None, None, None] ** 2 + 0.1)
    return score


def key(method, tol, row):
    return f"{method}_{tol:g}_row{row}"


def input_hash(y, z):
    h = hashlib.sha256()
    for v in (y, z):
        h.update(v.detach().contiguous().numpy().tobytes())
    return h.hexdigest()
