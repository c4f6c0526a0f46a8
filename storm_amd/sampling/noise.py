"""Noise source shared by the prior / predictor / corrector updates of one sampler run.

Default: counter-based Philox noise generated inside the update kernels — ``next`` only hands out
(seed, offset) pairs, so no noise tensor is ever materialised.  Parity runs inject the reference's
draws through ``noise_fn`` (draw order: prior, then per step the corrector draws followed by the
predictor draw — sampling/__init__.py:57-63).

``row_seeds`` = one Philox key per ROW of the batch instead of one seed for the call: row b then draws what a batch-1 run with
``seed = row_seeds[b]`` draws (the storm_*_rs kernels), so a seeded result does not depend on what the row is batched with.  The
key table is uploaded once, on the first draw, and handed out with every (seed, offset); the offset sequence is the same."""
import torch

from .. import ops


class NoiseSource:
    def __init__(self, seed=None, noise_fn=None, row_seeds=None):
        if row_seeds is not None and (seed is not None or noise_fn is not None):
            raise ValueError("row_seeds gives every row its own key: it cannot be combined with seed or noise_fn")
        if row_seeds is not None:
            row_seeds = ops.row_seed_table(row_seeds, "cpu")       # (checked here; uploaded on the first draw)
        if seed is None:
            seed = 0 if row_seeds is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
        self.seed, self.offset, self.noise_fn = int(seed), 0, noise_fn
        self.row_seeds, self._table = row_seeds, None

    def draw(self, like):
        """(z or None, keys) for one complex draw shaped like `like`; keys = the seed=, offset= (and row_seeds=) keywords of the
        update kernels (storm_amd.ops)"""
        z, seed, offset = self.next(like)
        keys = dict(seed=seed, offset=offset)
        if self.row_seeds is not None:
            if self._table is None or self._table.device != like.device:
                self._table = self.row_seeds.to(like.device)
            if self._table.shape[0] != like.shape[0]:
                raise ValueError(f"row_seeds has {self._table.shape[0]} keys for a batch of {like.shape[0]} rows")
            keys["row_seeds"] = self._table
        return z, keys

    def next(self, like):
        """returns (z or None, seed, offset) for one complex draw shaped like `like`"""
        if self.noise_fn is not None:
            z = self.noise_fn()
            if z.shape != like.shape:
                raise ValueError(f"injected noise has shape {tuple(z.shape)}, expected {tuple(like.shape)}")
            return z.to(device=like.device, dtype=torch.complex64).contiguous(), 0, 0
        self.offset += 1
        return None, self.seed, self.offset
