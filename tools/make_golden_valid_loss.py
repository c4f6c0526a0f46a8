"""Generate tests/golden/f23_valid_loss.npz: the REFERENCE's own `_step` (the number validation_step logs as valid_loss; model.py:138-154
ScoreModel, :329-349 DiscriminativeModel, :560-595 StochasticRegenerationModel) for every case of tests/valid_loss_cases.py.

Per case: torch.manual_seed(s) and the reference's `_step` on the seeded batch; the two draws of the step (rand, then randn_like) repeated
from the same seed and the step recomputed from them - asserted equal to `_step` bit for bit, so the recorded t (and the z the tests
regenerate from the seed) are the step's; the reference's fp32 loss(es); the same residual summed in fp64 per row; SHA-256 of the seeded
inputs, draws and weights; and the reference's OWN 16-bit error (its networks under torch.autocast in bf16 / fp16 on the CPU against its
fp32 loss), which bounds the engine's 16-bit tolerance as F22's does.

Runs only where the reference checkout exists (oracle.ref_import); tests read the .npz alone.

    python tools/make_golden_valid_loss.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402
from tests import valid_loss_cases as VC  # noqa: E402


def rows64(err, kind):
    """0.5 sum rho(err) per row in fp64 of the fp32 residual `err`"""
    e = (err.to(torch.complex128) if err.is_complex() else err.double()).abs().flatten(1)
    return 0.5 * (e ** 2 if kind == "mse" else e).sum(1)


def step_from_draws(m, kind, x, y, t, z, dt=None):
    """the reference's `_step` with its two draws handed in; returns (its return values, fp64 rows of the score loss, of the predictive loss).
    dt: the network calls (and only they) run under torch.autocast in that dtype - the SDE and the loss stay in fp32, as in the engine"""
    import contextlib

    def net(fn, *a):
        with (torch.autocast(device_type="cpu", dtype=dt) if dt is not None else contextlib.nullcontext()):
            o = fn(*a)
        return o.to(torch.complex64) if o.is_complex() else o.float()
    with torch.no_grad():
        if kind == "disc":
            xhat = net(m, y)
            loss = m._loss(x, xhat)
            if m.loss_type == "sisdr":
                s = m._istft(m._backward_transform(x.clone().squeeze(1))).double()
                sh = xhat.double()[..., :s.shape[-1]]
                s = s[..., :sh.shape[-1]]
                alpha = (sh * s).sum(-1, keepdim=True) / (s ** 2).sum(-1, keepdim=True)
                r = -10 * torch.log10(1e-10 + ((alpha * s) ** 2).sum(-1) / (1e-10 + ((alpha * s - sh) ** 2).sum(-1)))
            else:
                r = rows64(x - xhat, m.loss_type)
            return (loss,), None, r
        target = y if kind == "score" else net(m.forward_denoiser, y)
        mean, std = m.sde.marginal_prob(x, t, target)
        sig = std[:, None, None, None]
        xt = mean + sig * z
        if kind == "score":
            err = net(m, xt, t, y) * sig + z
            return (m._loss(err),), rows64(err, m.loss_type), None
        cond = {"noisy": [y], "post_denoiser": [target], "both": [y, target]}[m.condition]
        err = net(m.forward_score, xt, t, cond, target) * sig + z
        out = m._loss(err, target, x)
        return out, rows64(err, m.loss_type_score), (None if out[2] is None else rows64(target - x, m.loss_type_denoiser))


def main():
    ref = import_reference()
    M, DM = ref["model"], ref["data_module"].SpecsDataModule
    classes = {"score": M.ScoreModel, "disc": M.DiscriminativeModel, "storm": M.StochasticRegenerationModel}
    nan = float("nan")
    out = {}
    for name, (kind, kw, _) in VC.CASES.items():
        m, vals = VC.build(name, classes, data_module_cls=DM)
        x, y = VC.inputs(name)
        torch.manual_seed(VC.draw_seed(name))
        with torch.no_grad():
            got = m._step((x, y), 0)
        got = got if isinstance(got, tuple) else (got,)
        u, z = VC.draws(name)
        t = u * (m.sde.T - m.t_eps) + m.t_eps                       # model.py:144
        again, r_score, r_pred = step_from_draws(m, kind, x, y, t, z)
        for a, b in zip(got, again):                                # the recorded draws ARE the step's: bit for bit
            assert (a is None and b is None) or torch.equal(a, b), (name, a, b)
        loss = np.array([nan if v is None else float(v) for v in got], dtype=np.float32)
        assert np.isfinite(loss[0])
        out[f"{name}_loss"] = loss
        if r_score is not None:
            out[f"{name}_rows64_score"] = r_score.numpy()
            out[f"{name}_t"] = t.numpy()
            out[f"{name}_sha_draws"] = VC.sha([u, z])
        if r_pred is not None:
            out[f"{name}_rows64_pred"] = r_pred.numpy()
        out[f"{name}_sha_inputs"] = VC.sha([x, y])
        out[f"{name}_sha_weights"] = VC.sha(vals)
        line = f"{name}: loss {[float(v) for v in loss]}"
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
            l16, _, _ = step_from_draws(m, kind, x, y, t, z, dt=dt)
            err = max(abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(l16, got) if b is not None)
            out[f"{name}_referr_{tag}"] = np.float64(err)
            line += f", reference in {tag} {err:.2e}"
        print(line)
    path = os.path.join(ROOT, "tests", "golden", "f23_valid_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
