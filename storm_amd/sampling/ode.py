"""Probability-flow ODE sampler — drop-in for get_ode_sampler (sgmse/sampling/__init__.py:71-141).

The reference integrates dx/dt = theta (y - x) - 1/2 g(t)^2 score(x, t, y) from T to eps with
scipy.integrate.solve_ivp(RK45, rtol = atol = 1e-5) on a flattened host copy of the state (one
device <-> host round trip per right-hand side).  Here the solver state lives on the device:
an explicit Dormand-Prince 5(4) integrator with scipy's step-size controller (same error norm,
safety factor 0.9, growth limits [0.2, 10], same initial-step heuristic), so the accepted steps and
the number of function evaluations follow scipy's.  The solver algebra runs in fused HIP kernels (one pass per
Runge-Kutta stage, one for the scaled error norm); every right-hand side is one NCSN++ evaluation on the HIP engine
plus one fused drift pass; the host reads the per-row error sums once per attempted step.

Batches.  solve_ivp sees ONE flattened state, so `get_ode_sampler(sde, score_fn, y)` over a batch couples its rows through
the error norm exactly like the reference function does (per_row=False, the default: reference semantics for whatever
batch it is handed).  The reference MODEL never hands it more than one utterance (model.py:224-244, minibatch = 1): every
utterance has its own accepted / rejected step sequence.  per_row=True keeps that inside a batch: every row has its own
t, h, error norm and accept / reject decision, so row b of a batched run equals the batch-1 run of utterance b - this is
what ScoreModel.enhance_batch uses.  A row that has reached eps LEAVES the batch (compact=True, the default with per_row):
its end state is set aside and the state tensors shrink to the rows still integrating, so the network is never evaluated
on a finished row (compact=False: finished rows idle with h = 0 until the slowest row is done - the round-5 behaviour).

Methods.  The reference hands `method` on to solve_ivp.  The step loop here is a function of a Tableau record (C, A, B, the error
rows, n_stages, order, error_estimator_order), and solve_ivp's three explicit Runge-Kutta methods are records: RK45 (the default),
RK23 (Bogacki-Shampine 3(2): 3 evaluations per attempted step - the cheap one at loose tolerances) and DOP853 (Dormand-Prince 8(5,3):
12 per step, two error estimators combined on the host as scipy's _estimate_error_norm does).  RK45 and RK23 run through the 7-term
kernels, DOP853 through the wide forms (storm_rk_combine_rows_wide, storm_rk_error_pair_rows: 13 stages, both estimator sums in one
pass).  DOP853's order-8 estimate can sit in the fp32 rounding noise of the right-hand side (tight tolerances, a start state of
zero): its step sequence is then decided by that noise, in scipy as here, and evaluation counts agree only to a step.  The implicit
methods (Radau, BDF, LSODA) and solver classes are not implemented: NotImplementedError naming them.
"""
import collections
import math

import numpy as np
import torch

from .predictors import ReverseDiffusionPredictor

# Dormand-Prince coefficients (scipy.integrate._ivp.rk.RK45)
_C = [0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1]
_A = [[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9],
      [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
      [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]]
_B = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]
_E = [-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40]
_SAFETY, _MIN_FACTOR, _MAX_FACTOR = 0.9, 0.2, 10.0

# scipy.integrate._ivp.dop853_coefficients (C[:12], A[:12, :12], B, E3, E5; the dense-output rows are not needed), as literals
_DOP853_C = [0.0, 0.05260015195876773, 0.0789002279381516, 0.1183503419072274, 0.2816496580927726, 0.3333333333333333, 0.25,
             0.3076923076923077, 0.6512820512820513, 0.6, 0.8571428571428571, 1.0]
_DOP853_A = [[],
             [0.05260015195876773],
             [0.0197250569845379, 0.0591751709536137],
             [0.02958758547680685, 0.0, 0.08876275643042054],
             [0.2413651341592667, 0.0, -0.8845494793282861, 0.924834003261792],
             [0.037037037037037035, 0.0, 0.0, 0.17082860872947386, 0.12546768756682242],
             [0.037109375, 0.0, 0.0, 0.17025221101954405, 0.06021653898045596, -0.017578125],
             [0.03709200011850479, 0.0, 0.0, 0.17038392571223998, 0.10726203044637328, -0.015319437748624402, 0.008273789163814023],
             [0.6241109587160757, 0.0, 0.0, -3.3608926294469414, -0.868219346841726, 27.59209969944671, 20.154067550477894,
              -43.48988418106996],
             [0.47766253643826434, 0.0, 0.0, -2.4881146199716677, -0.590290826836843, 21.230051448181193, 15.279233632882423,
              -33.28821096898486, -0.020331201708508627],
             [-0.9371424300859873, 0.0, 0.0, 5.186372428844064, 1.0914373489967295, -8.149787010746927, -18.52006565999696,
              22.739487099350505, 2.4936055526796523, -3.0467644718982196],
             [2.273310147516538, 0.0, 0.0, -10.53449546673725, -2.0008720582248625, -17.9589318631188, 27.94888452941996,
              -2.8589982771350235, -8.87285693353063, 12.360567175794303, 0.6433927460157636]]
_DOP853_B = [0.054293734116568765, 0.0, 0.0, 0.0, 0.0, 4.450312892752409, 1.8915178993145003, -5.801203960010585, 0.3111643669578199,
             -0.1521609496625161, 0.20136540080403034, 0.04471061572777259]
_DOP853_E3 = [-0.18980075407240762, 0.0, 0.0, 0.0, 0.0, 4.450312892752409, 1.8915178993145003, -5.801203960010585, -0.4226823213237919,
              -0.1521609496625161, 0.20136540080403034, 0.02265179219836082, 0.0]
_DOP853_E5 = [0.01312004499419488, 0.0, 0.0, 0.0, 0.0, -1.2251564463762044, -0.4957589496572502, 1.6643771824549864, -0.35032884874997366,
              0.3341791187130175, 0.08192320648511571, -0.022355307863886294, 0.0]


class Tableau(collections.namedtuple("Tableau", "name C A B E n_stages order error_estimator_order")):
    """One explicit Runge-Kutta method of solve_ivp as the step loop reads it: the nodes C, the stage rows A (row s: its s
    coefficients), the weights B, the error-estimator rows E over K[0..n_stages] (one row: the embedded error; two, E5 and E3:
    DOP853's pair), and scipy's class attributes n_stages / order / error_estimator_order.  An attempted step costs n_stages
    evaluations (the first stage is the last one of the step before); the step-size exponents follow from error_estimator_order."""
    __slots__ = ()

    @property
    def error_exponent(self):
        return -1.0 / (self.error_estimator_order + 1)

    @property
    def wide(self):                                           # more stages than the 7-term entry points take
        return self.n_stages + 1 > 7


RK45 = Tableau("RK45", _C, _A, _B, (_E,), 6, 5, 4)
RK23 = Tableau("RK23", [0, 1 / 2, 3 / 4], [[], [1 / 2], [0, 3 / 4]], [2 / 9, 1 / 3, 4 / 9], ([5 / 72, -1 / 12, -1 / 9, 1 / 8],), 3, 3, 2)
DOP853 = Tableau("DOP853", _DOP853_C, _DOP853_A, _DOP853_B, (_DOP853_E5, _DOP853_E3), 12, 8, 7)
TABLEAUX = {tb.name: tb for tb in (RK45, RK23, DOP853)}
_ERR_EXP = RK45.error_exponent                                # (the default method's -1/5 under the name it had before the records)


def error_norm(tb, sums, h, n):
    """scipy's _estimate_error_norm from the scaled sums of squares over a solver state of n complex elements.  One estimator: the
    kernel has applied h, norm = sqrt(sum / n).  DOP853 (sums = (s5, s3), formed WITHOUT h): 0 if both are 0, else
    |h| s5 / sqrt((s5 + 0.01 s3) n)."""
    if len(tb.E) == 1:
        return math.sqrt(sums[0] / n)
    s5, s3 = sums
    if s5 == 0 and s3 == 0:
        return 0.0
    return abs(h) * s5 / math.sqrt((s5 + 0.01 * s3) * n)


def get_ode_sampler(sde, score_fn, y, inverse_scaler=None, denoise=True, rtol=1e-5, atol=1e-5, method="RK45",
                    eps=3e-2, device=None, noise_fn=None, seed=None, conditioning=None, per_row=False, compact=True, row_seeds=None,
                    **kwargs):
    """Probability-flow ODE sampler: an explicit Runge-Kutta method with scipy's step controller (solve_ivp's `RK45`, `RK23` or
    `DOP853` - method=, as the reference passes it on; sampling/__init__.py:71-141 runs them on the host over the flattened COMPLEX
    state: its norms are ||v|| / sqrt(n) over the n complex elements).  Everything per element runs in HIP kernels: one fused pass per
    stage (storm_rk_combine_rows / _wide) and one for the scaled error sums (storm_rk_scaled_sumsq_rows / storm_rk_error_pair_rows);
    the host reads the row sums once per attempted step (they decide acceptance) - no per-stage synchronisation.
    rtol, atol: the controller's tolerances; an attempted step costs the method's n_stages evaluations (6, 3, 12).
    per_row: one step controller per row instead of one for the whole batch (module docstring).
    compact (per_row only): rows that reached eps leave the batch instead of idling in every further evaluation.
    row_seeds: one Philox key per row for the prior draw (row b starts from what its batch-1 run with seed = row_seeds[b] starts
    from); the draw is made on the whole batch, before any row leaves it.
    Returns fn() -> (x, nfe); nfe = score evaluations executed; fn.nfev_rows = evaluations each row needed on its own;
    fn.rows_evaluated = rows summed over the executed evaluations (what the network really computed)."""
    if not isinstance(method, str) or method not in TABLEAUX:
        raise NotImplementedError(f"ODE method {method!r}: the explicit methods {sorted(TABLEAUX)} are implemented on the device")
    tb = TABLEAUX[method]
    from .. import ops
    # (RK45 and RK23 go through the 7-term entry points; DOP853's 12-term stages and 13-term estimator pair through the wide forms)
    combine = ops.rk_combine_rows_wide if tb.wide else ops.rk_combine_rows
    from .noise import NoiseSource
    noise = NoiseSource(seed=seed, noise_fn=noise_fn, row_seeds=row_seeds)
    predictor = ReverseDiffusionPredictor(sde, score_fn, probability_flow=False, noise=noise)
    rsde = sde.reverse(score_fn, probability_flow=True)

    def ode_sampler(z=None, **unused):
        with torch.no_grad():
            yy = y.contiguous()
            B = yy.shape[0]
            n_row = yy.numel() // B
            groups = [[b] for b in range(B)] if per_row else [list(range(B))]
            G = len(groups)
            shrink = bool(compact) and per_row and B > 1
            executed = rows_evaluated = 0
            # what the right-hand side reads besides x: the rows still integrating (all of them until a row leaves)
            y_c, cond_c = yy, conditioning

            def rows(vals):                                   # per group -> per row
                return [vals[g] for g, ids in enumerate(groups) for _ in ids]

            def f(t_g, x):
                nonlocal executed, rows_evaluated
                executed += 1
                rows_evaluated += x.shape[0]
                t_host = torch.tensor(rows(t_g), dtype=torch.float32)
                vec_t = t_host.to(yy.device)
                score = rsde._score(x, vec_t, (y_c,), dict(conditioning=cond_c))
                return sde.pf_drift(x, y_c, score.contiguous(), t_host)      # fused: a (y - x) - 1/2 g^2 score in one pass

            def norms(sumsq_rows):                            # scipy: ||v|| / sqrt(size) per solver state; ONE host read
                s = sumsq_rows.cpu().tolist()
                return [math.sqrt(sum(s[b] for b in ids) / (n_row * len(ids))) for ids in groups]

            def error_norms(x_new, K, hr, h):                 # the method's _estimate_error_norm per solver state; ONE host read
                # one estimator: the kernel multiplies by the rows' step sizes hr (scipy: norm(K.E h / scale)).  DOP853: the two sums
                # are formed without a step size (h_rows = None) and error_norm applies |h| once, to their quotient, as scipy does
                if len(tb.E) == 1:
                    s = [ops.rk_scaled_sumsq_rows(x, x_new, K, tb.E[0], hr, atol, rtol).cpu().tolist()]
                else:
                    s = ops.rk_error_pair_rows(x, x_new, K, tb.E[0], tb.E[1], None, atol, rtol).cpu().tolist()
                return [error_norm(tb, [sum(se[b] for b in ids) for se in s], h[g], n_row * len(ids)) for g, ids in enumerate(groups)]

            zz, keys = noise.draw(yy)
            # (a caller's start state is cloned: accepted rows are copied into x32 in place, and the caller may reuse z)
            x32 = sde.prior_sampling(yy.shape, yy, z=zz, **keys).contiguous() if z is None else z.contiguous().clone()
            x = x32.to(torch.complex128)                      # the solver state is complex128, as in scipy (module docstring)
            t_end, direction = float(eps), -1.0
            t = [float(sde.T)] * G
            f0 = f(t, x32)
            # scipy's select_initial_step, per solver state (three scalars each, once)
            d0 = norms(ops.rk_scaled_sumsq_rows(x, None, [], None, None, atol, rtol, mode=-3))
            d1 = norms(ops.rk_scaled_sumsq_rows(x, None, [f0], None, None, atol, rtol, mode=-1))
            h0 = [1e-6 if (d0[g] < 1e-5 or d1[g] < 1e-5) else 0.01 * d0[g] / d1[g] for g in range(G)]
            x1 = ops.rk_combine_rows(x, [f0], [1.0], rows([h * direction for h in h0]))
            f1 = f([t[g] + h0[g] * direction for g in range(G)], x1)
            d2 = norms(ops.rk_scaled_sumsq_rows(x, None, [f1, f0], None, None, atol, rtol, mode=-2))
            h_abs = []
            for g in range(G):
                dd2 = d2[g] / h0[g]
                h1 = max(1e-6, h0[g] * 1e-3) if (d1[g] <= 1e-15 and dd2 <= 1e-15) else (0.01 / max(d1[g], dd2)) ** (1 / (tb.error_estimator_order + 1))
                h_abs.append(min(100 * h0[g], h1))
            nfev = [2] * G
            fk = f0
            new_step, rejected = [True] * G, [False] * G
            min_step = [0.0] * G
            active = [(t[g] - t_end) * direction < 0 for g in range(G)]
            # compaction (per_row): `orig[g]` = the batch row that solver state g integrates; finished rows are parked in x_done
            orig = list(range(G))
            x_done, nfev_done = None, [0] * G
            while any(active):
                h, t_new = [0.0] * G, list(t)
                for g in range(G):
                    if not active[g]:
                        continue
                    if new_step[g]:                           # RungeKutta._step_impl's preamble
                        min_step[g] = 10 * abs(np.nextafter(t[g], direction * np.inf) - t[g])
                        h_abs[g] = max(h_abs[g], min_step[g])
                        new_step[g], rejected[g] = False, False
                    if h_abs[g] < min_step[g]:
                        raise RuntimeError("ODE step size underflow")
                    tn = t[g] + h_abs[g] * direction
                    if direction * (tn - t_end) > 0:
                        tn = t_end
                    t_new[g], h[g] = tn, tn - t[g]
                    h_abs[g] = abs(h[g])
                    nfev[g] += tb.n_stages
                hr = rows(h)                                  # (idle rows: h = 0, the stages leave them where they are)
                K = [fk]
                for s in range(1, tb.n_stages):
                    K.append(f([t[g] + tb.C[s] * h[g] for g in range(G)], combine(x, K, tb.A[s][:s], hr)))
                x_new, x_new32 = combine(x, K, tb.B, hr, want64=True)
                f_new = f(t_new, x_new32)
                K.append(f_new)
                err = error_norms(x_new, K, hr, h)
                accept = [False] * G
                for g in range(G):
                    if not active[g]:
                        continue
                    e = err[g]
                    if e < 1:
                        factor = _MAX_FACTOR if e == 0 else min(_MAX_FACTOR, _SAFETY * e ** tb.error_exponent)
                        if rejected[g]:
                            factor = min(1.0, factor)
                        h_abs[g] *= factor
                        accept[g], new_step[g] = True, True
                        t[g] = t_new[g]
                        active[g] = (t[g] - t_end) * direction < 0
                    else:
                        h_abs[g] *= max(_MIN_FACTOR, _SAFETY * e ** tb.error_exponent)
                        rejected[g] = True
                if all(accept):
                    x, x32, fk = x_new, x_new32, f_new
                elif any(accept):                             # the accepted rows move on; the others retry from where they are
                    acc_rows = rows(accept)
                    ops.copy_rows(x, x_new, acc_rows)
                    ops.copy_rows(x32, x_new32, acc_rows)
                    fk = ops.copy_rows(fk.clone() if fk is f0 else fk, f_new, acc_rows)
                if shrink and not all(active) and any(active):
                    # rows that reached eps leave: park their end state, shrink every per-row tensor to the rows still integrating
                    if x_done is None:
                        x_done = torch.empty_like(yy, dtype=x32.dtype)
                    gone = [g for g in range(G) if not active[g]]
                    keep = [g for g in range(G) if active[g]]
                    x_done.index_copy_(0, torch.tensor([orig[g] for g in gone], device=yy.device),
                                       x32.index_select(0, torch.tensor(gone, device=yy.device)))
                    for g in gone:
                        nfev_done[orig[g]] = nfev[g]
                    ki = torch.tensor(keep, device=yy.device)
                    x, x32, fk, y_c = x.index_select(0, ki), x32.index_select(0, ki), fk.index_select(0, ki), y_c.index_select(0, ki)
                    if isinstance(cond_c, (list, tuple)):
                        cond_c = [c.index_select(0, ki) for c in cond_c]
                    elif torch.is_tensor(cond_c):
                        cond_c = cond_c.index_select(0, ki)
                    pick = lambda vals: [vals[g] for g in keep]
                    t, h_abs, nfev, new_step, rejected, min_step, active, orig = (pick(t), pick(h_abs), pick(nfev), pick(new_step),
                                                                                    pick(rejected), pick(min_step), pick(active), pick(orig))
                    G = len(keep)
                    groups = [[g] for g in range(G)]
            if x_done is not None:                            # the rows that were still in the batch at the end join the parked ones
                x_done.index_copy_(0, torch.tensor(orig, device=yy.device), x32)
                for g in range(G):
                    nfev_done[orig[g]] = nfev[g]
                x, nfev_rows = x_done, nfev_done
            else:
                x, nfev_rows = x32, rows(nfev)
            ode_sampler.nfev_rows = nfev_rows
            ode_sampler.rows_evaluated = rows_evaluated
            nfe = executed
            if denoise:
                vec_eps = torch.ones(B, device=yy.device) * eps
                _, x = predictor.denoise_fn(x, vec_eps, yy, conditioning=conditioning)
            if inverse_scaler is not None:
                x = inverse_scaler(x)
            return x, nfe

    ode_sampler.nfev_rows = None
    ode_sampler.rows_evaluated = None
    return ode_sampler
