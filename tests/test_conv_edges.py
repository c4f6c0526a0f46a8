"""storm_conv per OUTPUT ELEMENT, on the host simulation and on the device: every kernel family of conv_igemm.hip, conv_pipe.hip (both
tiles and split-K), conv_pipe128.hip, conv_duo.hip, conv_thin.hip and conv_narrow.hip, forced by its switch and CONFIRMED by
storm_conv_kernel_name, at image sizes around the 8- / 16- / 20-row tiles and the 32-pixel tile width, channel counts around a K chunk,
output channels around an octet, a wave's 64 and the 128- / 256-cout tiles (tests/conv_cases.py).

  * cases whose arithmetic is exact by construction (small integers, sparse -1 / 0 / +1 weights, power-of-two scales): the output is the
    float64 reference bit for bit, pad channels are zero, and the fused GroupNorm partials sum to the exact (sum, sum of squares);
  * the same cases with 8 and 3 pretend CUs, so a persistent workgroup walks several tiles;
  * impulse weights: an output channel is an input channel shifted by one tap, zero border, bit for bit;
  * Gaussian operands with and without a fused GroupNorm + SiLU: worst pixel, worst channel and worst element within MARGIN x what a
    plain float32 restatement shows against float64;
  * ops.pack_gn_ss against the table storm_gn_finalize_ss writes."""
import pytest
import torch

from tests import conv_cases as CC
from tests.backend import dev, setup_backend, switch  # noqa: F401


@pytest.fixture
def sim():
    """the host simulation alone: conv_duo.hip is compiled into it and into the profiling library, never into the product library
    (storm_amd/build.py), so its cases have no device run"""
    return setup_backend("sim")


def _params(backend, with_cus=False, with_gn=False):
    """(family, dtype[, cus]) of the families that exist on `backend` ("hip": on both backends, through the dev fixture; "sim": there only)"""
    out = []
    for fam, f in CC.FAMILIES.items():
        if (backend == "hip") != ("hip" in f.backends) or (with_cus and not CC.walk_specs(fam)):
            continue
        for dt in f.dtypes:
            for cus in (CC.walk_cus(fam) if with_cus else (None,)):
                for gn in ((True, False) if with_gn else (None,)):
                    if with_gn and CC.measured_spec(fam, gn) is None:
                        continue                                        # (conv_thin.hip takes no fused affine: nothing to measure)
                    extra = ((cus,) if with_cus else ()) + ((gn,) if with_gn else ())
                    tag = ([f"cus{cus}"] if with_cus else []) + ([("gn_silu" if gn else "plain")] if with_gn else [])
                    out.append(pytest.param(*((fam, dt) + extra), id="-".join([fam, CC.dt_id(dt)] + tag)))
    return out


def _tag(dev):
    return "device" if dev.type == "cuda" else "simulation"


def _call(dev, fam, c, switch, partials, silu=False):
    """one storm_conv call of a case under the family's switches -> (y, part or None) on the host; the kernel is confirmed by name FIRST"""
    from storm_amd import ops
    for name, value in CC.FAMILIES[fam].switches:
        switch(name, value)
    s, dt = c.spec, c.dt
    dd = lambda t: None if t is None else t.to(dev)  # noqa: E731
    k = 3 if s.taps == 9 else 1
    ss = ops.pack_gn_ss(c.gn_scale, c.gn_shift).to(dev) if c.gn_scale is not None else None
    segs = [ops.Seg(dd(c.xa), ops.pack_conv_weight(c.w.to(dev), dt), k * k, src_b=dd(c.xb), gn_ss=ss, gn_silu=silu)]
    if c.w2 is not None:
        segs.append(ops.Seg(dd(c.sa), ops.pack_conv_weight(c.w2.to(dev), dt), 1, src_b=dd(c.sb)))
    tb = dd(c.tb)
    kw = dict(bias=dd(c.bias), tbias=tb[:, 8:] if tb is not None else None, skip=dd(c.skip), scale=s.scale, out_f32=s.out_f32, outC=s.outC)
    # ONE argument block for the name and for the launch (as ops.conv builds it: partials buffer, split-K scratch), so the name
    # confirmed is that of the kernel that runs whatever a family's rule looks at
    import ctypes
    from storm_amd import _lib as L
    a, y = ops._conv_args(segs, s.Cout, **kw)
    part = None
    if partials:
        part = torch.zeros((a.B, L.lib().storm_conv_tiles(ctypes.byref(a)), a.outC, 2), dtype=torch.float32, device=y.device)
        a.gn_part = L.ptr(part)
    need = L.lib().storm_conv_splitk_bytes(ctypes.byref(a))
    if need > 0:
        ws = torch.empty((need,), dtype=torch.uint8, device=y.device)
        a.splitk_ws, a.splitk_ws_bytes = L.ptr(ws), need
    name = L.lib().storm_conv_kernel_name(ctypes.byref(a)).decode()
    assert name == CC.kernel_name(fam, dt, s, silu), f"{fam}: the table's case {s} runs {name}"
    L.check(L.lib().storm_conv(ctypes.byref(a), L.stream()), "storm_conv")
    return y.cpu(), (part.cpu() if partials else None)


def _first_wrong(y, want):
    bad = (y != want).nonzero()
    return f"{len(bad)} wrong of {want.numel()}, first at (b, y, x, cout) = {tuple(int(v) for v in bad[0])}: " \
           f"{float(y[tuple(bad[0])])} instead of {float(want[tuple(bad[0])])}"


def _check_exact(fam, c, y, part):
    """-> None, or what is wrong with the call"""
    s = c.spec
    store = torch.float32 if s.out_f32 else c.dt
    if y.dtype != store or tuple(y.shape) != (s.B, s.H, s.W, s.outC):
        return f"output {y.dtype} {tuple(y.shape)}"
    want = c.ref.to(store)
    if not torch.equal(y[..., :s.Cout], want):
        return "output: " + _first_wrong(y[..., :s.Cout], want)
    if s.outC > s.Cout and bool((y[..., s.Cout:] != 0).any()):
        return "pad channels: " + _first_wrong(y[..., s.Cout:], torch.zeros_like(y[..., s.Cout:]))
    if part is not None:
        got = part.double().sum(1)[:, :s.Cout]
        if not torch.equal(got, c.sums):
            bad = (got != c.sums).nonzero()
            b, co, which = (int(v) for v in bad[0])
            return f"partials: {len(bad)} wrong of {c.sums.numel()}, first at (b, cout, sum / sum of squares) = {(b, co, which)}: " \
                   f"{float(got[b, co, which])} instead of {float(c.sums[b, co, which])}"
    return None


def _run_exact(dev, fam, dt, specs, switch):
    failures = []
    for s in specs:
        c = CC.build_exact(s, dt)
        y, part = _call(dev, fam, c, switch, partials=fam not in CC.NO_PARTIALS)
        wrong = _check_exact(fam, c, y, part)
        if wrong:
            failures.append(f"{s}: {wrong}")
    for f in failures:
        print(f)
    assert not failures, f"{len(failures)} of {len(specs)} cases, the first: {failures[0]}"


# ---------------------------------------------------------------- exact cases -------------
def _exact(dev, fam, dt, switch):
    _run_exact(dev, fam, dt, CC.specs_of(fam, dt), switch)


@pytest.mark.parametrize("fam,dt", _params("hip"))
def test_exact_cases_equal_the_float64_reference(dev, fam, dt, switch):
    """every shape of the family's table: y[..., :Cout] == the float64 reference cast to the storage type, pad channels zero, the
    GroupNorm partials summed over the tiles == the exact (sum, sum of squares) per (image, channel)"""
    _exact(dev, fam, dt, switch)


@pytest.mark.parametrize("fam,dt", _params("sim"))
def test_exact_cases_equal_the_float64_reference_simulation_only(sim, fam, dt, switch):
    _exact(sim, fam, dt, switch)


def _walk(dev, fam, dt, cus, switch):
    switch("STORM_CONV_CUS", cus)
    _run_exact(dev, fam, dt, CC.walk_specs(fam, cus), switch)


@pytest.mark.parametrize("fam,dt,cus", _params("hip", with_cus=True))
def test_exact_cases_under_a_persistent_tile_walk(dev, fam, dt, cus, switch):
    """every case of the family's table in which a workgroup stores several tiles when the device pretends to have 8 CUs (virtual blocks
    above resident workgroups, as the launch code counts them), and multi-tile variants of the concat, fused-affine, block-tail and
    deep_k cases with even and odd chunk counts: the next tile's prefetch overlaps the epilogue, the ring and the patch-buffer parity
    are handed to the next tile.  3 CUs only for conv_narrow.hip: the other kernels round the count up to 8 (conv_cases.walk_cus)"""
    _walk(dev, fam, dt, cus, switch)


@pytest.mark.parametrize("fam,dt,cus", _params("sim", with_cus=True))
def test_exact_cases_under_a_persistent_tile_walk_simulation_only(sim, fam, dt, cus, switch):
    _walk(sim, fam, dt, cus, switch)


def _impulses(dev, fam, dt, switch):
    for c, placed in CC.build_impulses(fam, dt):
        y, _ = _call(dev, fam, c, switch, partials=False)
        want = c.ref.to(dt)
        for co, tap, ci, where in placed:
            assert torch.equal(y[..., co], want[..., co]), f"tap {tap} at cin {ci} ({where}) -> cout {co}: " + _first_wrong(y[..., co:co + 1], want[..., co:co + 1])
        assert torch.equal(y[..., :c.spec.Cout], want), _first_wrong(y[..., :c.spec.Cout], want)
        assert not bool((y[..., c.spec.Cout:] != 0).any())


@pytest.mark.parametrize("fam,dt", _params("hip"))
def test_impulse_weights_shift_one_input_channel(dev, fam, dt, switch):
    """one weight of +1 per output channel at (tap, cin), every tap at a cin of the first chunk, of the ragged last chunk and of the
    second operand of the concat: out[b, y, x, co] == in[b, y + dy, x + dx, cin] with a zero border - the orientation of the taps and
    the masking of the border as a reader checks them by eye"""
    _impulses(dev, fam, dt, switch)


@pytest.mark.parametrize("fam,dt", _params("sim"))
def test_impulse_weights_shift_one_input_channel_simulation_only(sim, fam, dt, switch):
    _impulses(sim, fam, dt, switch)


# ---------------------------------------------------------------- measured cases ----------
def _measured(dev, fam, dt, gn, switch):
    spec = CC.measured_spec(fam, gn)
    c = CC.build_measured(spec, dt)
    y, _ = _call(dev, fam, c, switch, partials=False, silu=True)
    assert torch.isfinite(y.float()).all()
    got = CC.figures(y[..., :spec.Cout], c.ref)
    bound = tuple(CC.MARGIN[dt] * v for v in c.own)
    print(f"conv {fam} {'gn+silu' if gn else 'plain'} {CC.dt_id(dt)} {_tag(dev)}: worst pixel {got[0]:.3e} (bound {bound[0]:.3e}, restatement "
          f"{c.own[0]:.3e}); worst channel {got[1]:.3e} (bound {bound[1]:.3e}, restatement {c.own[1]:.3e}); worst element {got[2]:.3e} "
          f"(bound {bound[2]:.3e}, restatement {c.own[2]:.3e})")
    assert all(g <= b for g, b in zip(got, bound)), (got, bound)
    assert not bool((y[..., spec.Cout:] != 0).any())


@pytest.mark.parametrize("fam,dt,gn", _params("hip", with_gn=True))
def test_gaussian_cases_within_the_plain_restatement(dev, fam, dt, gn, switch):
    """Gaussian operands at the family's edge shape, with a fused GroupNorm + SiLU and without: worst pixel (RMS over its couts), worst
    channel (RMS over its pixels) and worst element against float64, over the RMS of the reference, each within MARGIN x the figure of
    the plain float32 restatement"""
    _measured(dev, fam, dt, gn, switch)


@pytest.mark.parametrize("fam,dt,gn", _params("sim", with_gn=True))
def test_gaussian_cases_within_the_plain_restatement_simulation_only(sim, fam, dt, gn, switch):
    _measured(sim, fam, dt, gn, switch)


# ---------------------------------------------------------------- the table's layout ------
def test_pack_gn_ss_is_the_layout_gn_finalize_writes(dev, switch):
    """ops.pack_gn_ss(scale, shift) against the table ops.gn_finalize(..., gamma, beta, count) returns for a concat of two tensors:
    statistics of exact integer partials, gamma and beta different in every channel (a table in another order cannot agree)"""
    from storm_amd import ops
    dt = torch.bfloat16
    ca = CC.build_exact(CC.Spec(2, 9, 33, 72, 24), dt)
    cb = CC.build_exact(CC.Spec(2, 9, 33, 24, 40), dt)
    (ya, pa), (yb, pb) = (_call(dev, "igemm0" if c is ca else "igemm_small", c, switch, partials=True) for c in (ca, cb))
    C, count = 72 + 24, 9 * 33
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    _, ss = ops.gn_finalize(pa.to(dev), pb.to(dev), gamma=gamma.to(dev), beta=beta.to(dev), count=count)
    G = ops.gn_groups(C)
    sums = torch.cat([ca.sums, cb.sums], 1).reshape(2, G, C // G, 2).sum(2)           # exact (sum, sum of squares) per group
    mean = sums[..., 0] / (count * (C // G))
    rstd = 1.0 / torch.sqrt(sums[..., 1] / (count * (C // G)) - mean * mean + 1e-6)
    scale = rstd.repeat_interleave(C // G, 1) * gamma.double()
    shift = beta.double() - mean.repeat_interleave(C // G, 1) * scale
    want = ops.pack_gn_ss(scale, shift)
    assert ss.shape == want.shape == (2, C // 8, 2, 8)
    assert torch.allclose(ss.cpu(), want, rtol=1e-5, atol=1e-6), float((ss.cpu() - want).abs().max())
