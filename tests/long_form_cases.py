"""Helpers of tests/test_long_form.py: the numpy restatement of the stitch of include/storm_hip.h ("Long recordings"), the kernel cases and
the pipeline's own composition from enhance_batch calls."""
import numpy as np
import torch

GOLDEN = 0x9E3779B97F4A7C15


def ramp_ref(V, kind):
    """the ramp's definition in fp64, rounded to fp32 once"""
    j = np.arange(V, dtype=np.float64)
    r = np.sin(np.pi / 2 * (j + 1) / (V + 1)) ** 2 if kind == "hann" else (j + 1) / (V + 1)
    return r.astype(np.float32)


def plan_ref(L, W, V):
    """(n, padded length) of a recording of L > W samples"""
    H = W - V
    n = -(-(L - V) // H)
    return n, (n - 1) * H + W


def key_ref(key, k):
    return (key + (k + 1) * GOLDEN) % 2 ** 63


def stitch_ref(pool, rows, L, W, V, ramp, width):
    """One recording: pool float32 [N, W], rows = the pool row of each of its n windows (-1: skipped, reads as zeros), L samples ->
    float32 [width].  k = min(m // H, n - 1), j = m - k H; in the first V samples of a window with a predecessor
    out = prev + ramp[j] * (cur - prev), three float32 operations; cur otherwise; zero from L on."""
    H, n = W - V, len(rows)
    wins = np.stack([pool[r] if r >= 0 else np.zeros(W, np.float32) for r in rows]).astype(np.float32)
    m = np.arange(L)
    k = np.minimum(m // H, n - 1)
    j = m - k * H
    assert j.max() < W
    cur = wins[k, j]
    fade = (k > 0) & (j < V)
    prev = wins[np.maximum(k - 1, 0), np.where(fade, j + H, 0)]
    d = (cur - prev).astype(np.float32)
    p = (ramp[np.where(fade, j, 0)] * d).astype(np.float32)
    mixed = (prev + p).astype(np.float32)
    out = np.zeros(width, np.float32)
    out[:L] = np.where(fade, mixed, cur)
    return out


def random_pool(N, W, seed, stride=None):
    """float32 [N, W] of random values (NOT cut from one signal: cur != prev in every overlap); stride: the row stride of the tensor the
    pool is a view of"""
    g = torch.Generator().manual_seed(seed)
    big = torch.randn(N, stride or W, generator=g)
    return big[:, :W]


def launch_case(recs, W, V, seed, stride=None, permute=True, skip=(), extra_rows=1):
    """recs = [L_0, L_1, ...] -> (pool, win_row, rec_len, rec_windows): a random pool whose rows are dealt to the windows in a seeded
    permutation (interleaving the recordings), `extra_rows` rows that no window names; skip = {(recording, window)} marked -1"""
    ns = [plan_ref(L, W, V)[0] if L > W else 1 for L in recs]
    total = sum(ns)
    N = total + extra_rows
    order = np.random.default_rng(seed).permutation(N)[:total] if permute else np.arange(total)
    win_row, at = [], 0
    for r, n in enumerate(ns):
        for k in range(n):
            win_row.append(-1 if (r, k) in skip else int(order[at]))
            at += 1
    return random_pool(N, W, seed, stride), win_row, list(recs), ns


def launch_ref(pool, win_row, rec_len, rec_windows, W, V, ramp, width):
    p = pool.cpu().numpy()
    out, at = [], 0
    for L, n in zip(rec_len, rec_windows):
        out.append(stitch_ref(p, win_row[at:at + n], L, W, V, ramp, width))
        at += n
    return np.stack(out)


def compose(model, wav, key, W, V, ramp, call):
    """The pipeline's definition for ONE 16 kHz recording from existing calls: every window alone through `call(rows [1, W], peak [1],
    row_seeds [1]) -> [1, W]` with the RECORDING's peak and ops.window_key, stitched in numpy.  wav: 1-D device tensor of more than W samples."""
    from storm_amd import ops
    L = wav.numel()
    n, padded = plan_ref(L, W, V)
    H = W - V
    buf = torch.zeros(padded, dtype=torch.float32, device=wav.device)
    buf[:L] = wav
    peak = ops.peak_abs(wav.reshape(1, -1))
    wins = [call(buf[k * H:k * H + W].reshape(1, -1), peak, [key_ref(key, k)]) for k in range(n)]
    pool = torch.cat(wins).cpu().numpy()
    return torch.from_numpy(stitch_ref(pool, list(range(n)), L, W, V, ramp_ref(V, ramp), L))
