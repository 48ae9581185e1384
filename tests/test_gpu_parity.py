"""GPU parity: HIP kernels (through the C ABI) against the CPU oracle on identical seeded inputs,
against the reference's golden checksums, and size-independent properties at full size.

Tolerances: fields are double precision; the GPU build contracts a*b+c into FMAs and the scatter
uses atomics (summation order differs), so element-wise agreement is ~1e-13 relative, far inside
the north-star budget of 1e-6; integer particle indexing (validity flags, cell indices) is exact.
"""
import json
import os

import numpy as np
import pytest

from hipace_amd import decks
from tests.util import G2, NCOMP, rel_err, smooth_slab, thermal_sheet

pytestmark = pytest.mark.gpu

LO, HI = (-8.0, -8.0), (8.0, 8.0)
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def _oracle_geom(O, nx, ny, dz=0.12, bc=1):
    return O.make_geom(nx, ny, LO, HI, dz=dz, bc=bc)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [64, 96])
def test_deposit_current(api, oracle, order, n):
    g = (order + 1) // 2 + 1
    real, valid, ion = thermal_sheet(n, n, LO, HI, ppc=2, seed=order + n)
    real[5, :7] = -0.3           # psi < 0 -> QSA violation -> particle dropped
    comp = [15, 16, 3, 18, 2, 17]
    ref = np.zeros((NCOMP, n + 2 * g, n + 2 * g))
    r2, v2 = real.copy(), valid.copy()
    nq = oracle.deposit_current(ref, n, n, g, r2, v2, ion, _oracle_geom(oracle, n, n), comp, -1.0, 1.0, order)
    f = api.Fields(n, n, g, NCOMP)
    pl = api.PlasmaSheet(real, valid, ion)
    import torch
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    api.DepositCurrent(pl, f, api.Geometry(n, n, LO, HI, 0.12), -1.0, 1.0, order, jx=15, jy=16, jz=3, rho=18, chi=2,
                       rhomjz=17, n_qsa=cnt)
    out = f.numpy()
    for c in comp:
        assert rel_err(out[c], ref[c]) < 1e-12, (c, rel_err(out[c], ref[c]))
    untouched = [c for c in range(NCOMP) if c not in comp]
    assert np.all(out[untouched] == 0.0)
    greal, gvalid = pl.numpy()
    assert int(cnt.item()) == nq == 7
    assert np.array_equal(gvalid, v2)                # integer state bit-exact
    assert np.array_equal(greal[2], r2[2])           # weights of dropped particles zeroed


@pytest.mark.parametrize("order,dtype", [(0, 2), (1, 2), (2, 2), (3, 2), (2, 1)])
def test_explicit_deposit(api, oracle, order, dtype):
    n = 64
    g = (order + 1) // 2 + 1
    real, valid, ion = thermal_sheet(n, n, LO, HI, ppc=2, seed=3)
    valid[::17] = 0
    slab = smooth_slab(n, n, g)
    ref = slab.copy()
    oracle.explicit_deposit(ref, n, n, g, real.copy(), valid.copy(), ion, _oracle_geom(oracle, n, n),
                            [10, 7, 5, 6], [3, 4], -1.0, 1.0, order, dtype)
    f = api.Fields(n, n, g, NCOMP, data=slab)
    pl = api.PlasmaSheet(real, valid, ion)
    api.ExplicitDeposition(pl, f, api.Geometry(n, n, LO, HI, 0.12), -1.0, 1.0, order, Bz=10, Ez=7, ExmBy=5, EypBx=6,
                           Sy=3, Sx=4, derivative_type=dtype)
    out = f.numpy()
    for c in (3, 4):
        assert rel_err(out[c], ref[c]) < 1e-12, (c, rel_err(out[c], ref[c]))
    rest = [c for c in range(NCOMP) if c not in (3, 4)]
    assert np.array_equal(out[rest], slab[rest])


@pytest.mark.parametrize("order,bc,nsc", [(o, b, 1) for o in (0, 1, 2, 3) for b in (0, 1, 2)] + [(2, 1, 2), (3, 0, 3), (1, 2, 2)])
def test_advance_plasma(api, oracle, order, bc, nsc):
    """nsc = <plasma>.n_subcycles (PlasmaParticleAdvance.cpp:92-217: the gather is repeated at the new position)."""
    n = 64
    g = (order + 1) // 2 + 1
    real, valid, ion = thermal_sheet(n, n, LO, HI, ppc=2, seed=11 + bc, u_std=0.3)
    valid[5::23] = 0
    # push the outermost particles across the wall so that every boundary type is exercised
    edge = (np.abs(real[6]) > 7.9) | (np.abs(real[7]) > 7.9)
    real[8][edge] = 3.0 * np.sign(real[6][edge])
    real[9][edge] = 3.0 * np.sign(real[7][edge])
    real[10][edge] = np.sqrt(1.0 + real[8][edge] ** 2 + real[9][edge] ** 2)
    slab = smooth_slab(n, n, g, amp=0.2)
    r2, v2 = real.copy(), valid.copy()
    oracle.advance_plasma(slab, n, n, g, r2, v2, ion, _oracle_geom(oracle, n, n, dz=0.4, bc=bc),
                          [11, 7, 8, 9, 10], -1.0, 1.0, order, n_subcycles=nsc)
    assert 0.1 < r2[5][v2 != 0].min() and r2[5].max() < 20.0     # well-conditioned inputs
    f = api.Fields(n, n, g, NCOMP, data=slab)
    pl = api.PlasmaSheet(real, valid, ion)
    api.AdvancePlasmaParticles(pl, f, api.Geometry(n, n, LO, HI, 0.4, bc=bc), -1.0, 1.0, order, Psi=11, Ez=7, Bx=8,
                               By=9, Bz=10, n_subcycles=nsc)
    greal, gvalid = pl.numpy()
    assert np.array_equal(gvalid, v2)
    if bc == 2:
        assert (v2 == 0).sum() > (valid == 0).sum()      # some particles were absorbed
    live = v2 != 0
    for k in range(11):
        assert rel_err(greal[k][live], r2[k][live]) < 1e-10, (k, rel_err(greal[k][live], r2[k][live]))
    assert np.array_equal(greal[2][~live], r2[2][~live])


@pytest.mark.parametrize("nx,ny", [(64, 64), (32, 48), (63, 63), (127, 65), (32, 64), (128, 32), (512, 512),
                                   (1024, 1024), (1023, 1023), (256, 256), (256, 100), (48, 500), (600, 520),
                                   (511, 511), (255, 255), (511, 127), (1023, 511), (2047, 255)])
# against the oracle: every length of the power-of-two kernel (2^6 .. 2^11), five of the seven lengths of the symmetric one,
# three of the four tridiagonal shapes (ny <= 1024); tests/test_poisson_dispatch_gpu.py reaches every kernel of the dispatch
def test_poisson(api, oracle, nx, ny):
    import torch
    rng = np.random.default_rng(nx * 1000 + ny)
    rhs = rng.standard_normal((ny, nx))
    dx, dy = 0.25, 0.2
    ref = oracle.poisson_solve(rhs, dx, dy)
    ps = api.FFTPoissonSolver(nx, ny, dx, dy)
    ps.StagingArea().copy_(torch.as_tensor(rhs))
    f = api.Fields(nx, ny, G2, 3)
    ps.SolvePoissonEquation(f, 1)
    out = f.numpy()
    assert rel_err(out[1, G2:-G2, G2:-G2], ref) < 1e-12
    assert np.all(out[0] == 0) and np.all(out[2] == 0)
    guards = out[1].copy()
    guards[G2:-G2, G2:-G2] = 0
    assert np.all(guards == 0)                          # guard cells are never written


def test_poisson_batch(api, oracle):
    """Three stacked solves (Psi, Ez, Bz of one slice) through the batched entry point."""
    import ctypes as C
    import torch
    from hipace_amd import _lib
    nx = ny = 64
    rng = np.random.default_rng(3)
    rhs = rng.standard_normal((3, ny, nx))
    dx = dy = 0.25
    ps = api.FFTPoissonSolver(nx, ny, dx, dy)
    st = torch.as_tensor(rhs).cuda().contiguous()
    f = api.Fields(nx, ny, G2, 6)
    comps = (C.c_int * 3)(4, 1, 2)
    _lib.check(_lib.lib().hps_poisson_solve_batch(ps._h, 3, C.c_void_p(st.data_ptr()), f.struct(), comps, None))
    torch.cuda.synchronize()
    out = f.numpy()
    for b, c in enumerate((4, 1, 2)):
        assert rel_err(out[c, G2:-G2, G2:-G2], oracle.poisson_solve(rhs[b], dx, dy)) < 1e-12
    assert np.all(out[[0, 3, 5]] == 0)


@pytest.mark.parametrize("nx,ny", [(64, 64), (32, 32), (96, 48), (63, 63), (31, 63), (512, 512), (1024, 1024), (1023, 1023), (511, 511), (255, 127),
                                   (132, 66), (2047, 2047)])
@pytest.mark.parametrize("warm", [False, True])
def test_multigrid_solve1(api, oracle, nx, ny, warm):
    """Stand-alone hpmg solve1 against the oracle, up to the headline size (every kernel of the V-cycle: LDS-tiled
    smoothers of the fine levels, fused level-0 end pass, k_lower_v3 / k_lower_v) with equal V-cycle counts.  132 x 66 is a
    cell-centred grid whose coarsening stops at 66 x 33, too large for k_lower_v3: its lower V is k_lower_v<true>."""
    rng = np.random.default_rng(nx + 7 * ny)
    g = G2
    dx, dy = 16.0 / nx, 16.0 / ny
    slab = np.zeros((5, ny + 2 * g, nx + 2 * g))
    slab[2:4, g:-g, g:-g] = rng.standard_normal((2, ny, nx))              # rhs
    slab[4] = 0.5 + rng.random((ny + 2 * g, nx + 2 * g))                   # acoef (chi)
    if warm:
        slab[0:2, g:-g, g:-g] = 0.05 * rng.standard_normal((2, ny, nx))  # initial guess
    sol = np.ascontiguousarray(slab[0:2]).copy()
    it_ref, rn_ref = oracle.mg_solve1(sol, np.ascontiguousarray(slab[2:4]), np.ascontiguousarray(slab[4]), nx, ny, g, dx, dy)
    f = api.Fields(nx, ny, g, 5, data=slab)
    it, rn = api.MultiGrid(nx, ny, dx, dy).solve1(f, 0, 2, 4)
    out = f.numpy()
    assert it == it_ref and it_ref >= 1
    assert rel_err(out[0:2], sol) < 1e-10
    assert abs(rn - rn_ref) <= 1e-6 * rn_ref
    assert np.array_equal(out[2:5], slab[2:5])


def test_multigrid_solve1_with_the_references_argument_list(api, oracle):
    """hps_mg_solve1_fabs: hpmg::MultiGrid::solve1(sol, rhs, acoef, ...) with three separate fabs (HpMultiGrid.H:64-66), here with
    three different guard widths -- same V-cycle count and solution as the oracle, both centrings."""
    for nx, ny in ((96, 64), (63, 63)):
        rng = np.random.default_rng(nx)
        dx, dy = 16.0 / nx, 16.0 / ny
        rhs = rng.standard_normal((2, ny, nx))
        acf = 0.5 + rng.random((ny + 2 * G2, nx + 2 * G2))
        guess = 0.05 * rng.standard_normal((2, ny, nx))
        sol = np.zeros((2, ny + 2 * G2, nx + 2 * G2)); sol[:, G2:-G2, G2:-G2] = guess
        rhs_g = np.zeros_like(sol); rhs_g[:, G2:-G2, G2:-G2] = rhs
        it_ref, rn_ref = oracle.mg_solve1(sol, rhs_g, acf, nx, ny, G2, dx, dy)
        gs, gr, ga = 1, 3, G2                                  # guard cells of the three views
        fs = api.Fields(nx, ny, gs, 2); fs.t[:, gs:-gs, gs:-gs] = __import__("torch").tensor(guess, device="cuda")
        fr = api.Fields(nx, ny, gr, 2); fr.t[:, gr:-gr, gr:-gr] = __import__("torch").tensor(rhs, device="cuda")
        fa = api.Fields(nx, ny, ga, 1, data=acf[None])
        it, rn = api.MultiGrid(nx, ny, dx, dy).solve1_fabs(fs, fr, fa)
        assert it == it_ref and it_ref >= 1
        assert rel_err(fs.numpy()[:, gs:-gs, gs:-gs], sol[:, G2:-G2, G2:-G2]) < 1e-10
        assert abs(rn - rn_ref) <= 1e-6 * rn_ref


@pytest.mark.parametrize("name,js", [("linear_wake_SI", "linear_wake.SI.1Rank"), ("beam_in_vacuum_SI", "beam_in_vacuum.SI.1Rank"),
                                     ("linear_wake", "linear_wake.normalized.1Rank"),
                                     ("blowout_wake", "blowout_wake_explicit.2Rank"), ("blowout_wake", "blowout_wake.2Rank"),
                                     ("beam_in_vacuum", "beam_in_vacuum.normalized.Serial"),
                                     ("beam_in_vacuum_1Rank", "beam_in_vacuum.normalized.1Rank"),
                                     ("beam_in_vacuum_SI_Serial", "beam_in_vacuum.SI.Serial"),
                                     ("grid_current", "grid_current.1Rank"), ("reset", "reset.2Rank"),
                                     # boundary.field = Open with the predictor-corrector loop, order 0, an off-centre beam
                                     ("beam_in_vacuum_open_boundary", "beam_in_vacuum_open_boundary.normalized.1Rank"),
                                     ("gaussian_linear_wake", "gaussian_linear_wake.normalized.1Rank"),
                                     ("gaussian_linear_wake_SI", "gaussian_linear_wake.SI.1Rank")])
def test_engine_reproduces_reference_checksums(api, name, js):
    """North-star parity bar: field checksums within 1e-6 of the reference's CPU goldens."""
    gold = json.load(open(os.path.join(GOLD, js + ".json")))["lev=0"]
    eng = api.SliceEngine(decks.NAMED[name]())
    eng.set_diagnostics(True)
    for _ in range(eng.deck["n_steps"]):
        eng.run_step()
    cs = eng.checksums()
    for k, v in gold.items():
        if v == 0.0:
            assert cs[k] == 0.0, k
        else:
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (k, cs[k], v)


@pytest.mark.parametrize("tile_size", [0, 16])
def test_engine_slice_by_slice_vs_oracle(api, oracle, tile_size):
    deck = decks.blowout_wake()
    deck.update(nz=40, n_steps=1)
    ge = api.SliceEngine(deck, tile_size=tile_size, sort_period=5)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    from hipace_amd._lib import COMPS
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        if isl % 13 == 0:
            gs, os_ = ge.slab(), oe.slab()
            for c in range(ge.ncomp):
                assert rel_err(gs[c], os_[c]) < 1e-9, (isl, COMPS[c], rel_err(gs[c], os_[c]))
    greal, gvalid = ge.particles()
    oreal, ovalid = oe.particles()
    if tile_size:      # the tiled engine keeps the sheet in tile order: compare as sets
        gk = np.lexsort((np.round(greal[0], 7), np.round(greal[1], 7)))
        ok = np.lexsort((np.round(oreal[0], 7), np.round(oreal[1], 7)))
        greal, gvalid, oreal, ovalid = greal[:, gk], gvalid[gk], oreal[:, ok], ovalid[ok]
    assert np.array_equal(gvalid, ovalid)
    for k in range(11):
        assert rel_err(greal[k], oreal[k]) < 1e-9, k
    assert ge.stats()["vcycles"] == oe.vcycles()


def test_full_size_properties(api):
    """1024^2, 4 ppc (BASELINE config 4 transverse size): properties that need no oracle run."""
    import torch
    n, g = 1024, G2
    real, valid, ion = thermal_sheet(n, n, LO, HI, ppc=2, seed=99)
    geom = api.Geometry(n, n, LO, HI, 12.0 / 1024)
    f = api.Fields(n, n, g, NCOMP)
    pl = api.PlasmaSheet(real, valid, ion)
    # charge conservation: sum of deposited rhomjz == sum q w (normalised units, invvol = 1)
    api.DepositCurrent(pl, f, geom, -1.0, 1.0, 2, rhomjz=17, chi=2)
    tot = f.t[17].sum().item()
    assert abs(tot - (-real[2].sum())) < 1e-9 * real[2].sum()
    # linearity: depositing twice doubles the field
    once = f.t[17].clone()
    api.DepositCurrent(pl, f, geom, -1.0, 1.0, 2, rhomjz=17)
    assert torch.allclose(f.t[17], 2 * once, rtol=1e-12, atol=1e-14)
    # Poisson: 5-point Laplacian of the solution returns the source
    ps = api.FFTPoissonSolver(n, n, geom.c.dx, geom.c.dy)
    src = once[g:-g, g:-g].contiguous()
    ps.StagingArea().copy_(src)
    api_f = api.Fields(n, n, g, 1)
    ps.SolvePoissonEquation(api_f, 0)
    F = api_f.t[0]
    lap = ((F[g:-g, g + 1:n + g + 1] + F[g:-g, g - 1:n + g - 1] - 2 * F[g:-g, g:-g]) / geom.c.dx ** 2
           + (F[g + 1:n + g + 1, g:-g] + F[g - 1:n + g - 1, g:-g] - 2 * F[g:-g, g:-g]) / geom.c.dy ** 2)
    assert (lap - src).abs().max().item() < 1e-6 * src.abs().max().item()   # conditioning ~ n^2 * eps
    # multigrid: reported residual norm meets the tolerance and the residual really is that small
    f2 = api.Fields(n, n, g, 5)
    f2.t[2:4, g:-g, g:-g] = torch.randn((2, n, n), dtype=torch.float64, device="cuda",
                                        generator=torch.Generator(device="cuda").manual_seed(5))
    f2.t[4] = 0.5 + torch.rand((n + 2 * g, n + 2 * g), dtype=torch.float64, device="cuda",
                               generator=torch.Generator(device="cuda").manual_seed(6))
    it, rn = api.MultiGrid(n, n, geom.c.dx, geom.c.dy).solve1(f2, 0, 2, 4, tol_rel=1e-8)
    assert 1 <= it <= 12
    S, R, A = f2.t[0:2], f2.t[2:4], f2.t[4]
    fx, fy = 1 / geom.c.dx ** 2, 1 / geom.c.dy ** 2
    c = slice(g + 1, n + g - 1)       # interior cells (wall cells use the 4/3-2 stencil)
    lap = (fx * (S[:, c, g + 2:n + g] + S[:, c, g:n + g - 2] - 2 * S[:, c, c])
           + fy * (S[:, g + 2:n + g, c] + S[:, g:n + g - 2, c] - 2 * S[:, c, c]))
    res = R[:, c, c] + A[c, c] * S[:, c, c] - lap
    assert res.abs().max().item() <= 1e-8 * R.abs().max().item() * 1.0001


@pytest.mark.parametrize("n,nsl", [(512, 6), (1024, 3), (1023, 3), (511, 5), (2047, 3)])
def test_baseline_blowout_configs_head_slices(api, oracle, n, nsl):
    """BASELINE configs 3 and 4 at their full transverse size (blowout_wake n x n x 1024, 4 ppc, explicit solver) -- and the
    grid the reference recommends, 2^N - 1 = 1023 and 2047 cells per side (docs/source/run/parameters.rst:313-321: length-1024
    and -2048 transforms, node-centred multigrid coarsening; at 2047 the y solves are k_tridiag_y<32, 8>) --:
    a few slices through the driver against the oracle -- every slab component and the V-cycle count.  Both engines
    start on a slice one sigma ahead of the beam centre (the static beam blocks are addressed by slice), where the
    fields are strong from the first slice on.  (The whole box would take the oracle 20 min to 1 h; the decks'
    whole-box checksums are covered at 64^2 by the golden fixtures.)"""
    from hipace_amd._lib import COMPS
    deck = decks.synthetic(n, 1024, 2)
    ge = api.SliceEngine(deck, tile_size=16, sort_period=128)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    for isl in range(640, 640 - nsl, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
    gs, os_ = ge.slab(), oe.slab()
    assert np.abs(os_[COMPS.index("Bx")]).max() > 1e-2 and np.abs(os_[COMPS.index("Ez")]).max() > 1e-4
    for c in range(ge.ncomp):
        assert rel_err(gs[c], os_[c]) < 1e-8, (COMPS[c], rel_err(gs[c], os_[c]))
    assert ge.stats()["vcycles"] == oe.vcycles()


# ------------------------------------------------------------------------------------------------
# tile-sorted sheet: sort is bit-exact against the CPU restatement; LDS-tile kernels agree with
# the oracle both for a fresh sort and for a stale one (particles far outside their home tile)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [16, 32])
@pytest.mark.parametrize("n", [64, 100])
def test_tile_sort_bit_exact(api, oracle, ts, n):
    real, valid, ion = thermal_sheet(n, n, LO, HI, ppc=2, seed=ts + n, jitter=9.0)
    valid[3::11] = 0
    geom = api.Geometry(n, n, LO, HI, 0.12)
    til = api.Tiling(n, n, ts, real.shape[1])
    out = til.reorder(api.PlasmaSheet(real, valid, ion), geom)
    off, perm = til.offsets_and_perm(real.shape[1])
    operm, ooff = oracle.tile_sort(real, valid, ion, _oracle_geom(oracle, n, n), n, n, ts)
    assert np.array_equal(perm, operm)              # integer work: bit-exact
    assert np.array_equal(off, ooff)
    greal, gvalid = out.numpy()
    assert np.array_equal(greal, real[:, operm])    # pure data movement: bit-exact
    assert np.array_equal(gvalid, valid[operm])


@pytest.mark.parametrize("ts", [16, 32])
@pytest.mark.parametrize("stale", [False, True])
@pytest.mark.parametrize("order", [0, 2, 3])
def test_tiled_operators(api, oracle, ts, stale, order):
    import torch
    n = 96
    g = (order + 1) // 2 + 1
    real, valid, ion = thermal_sheet(n, n, LO, HI, ppc=2, seed=5 + order, u_std=0.3)
    valid[7::29] = 0
    geom = api.Geometry(n, n, LO, HI, 0.3)
    ogeom = _oracle_geom(oracle, n, n, dz=0.3)
    til = api.Tiling(n, n, ts, real.shape[1])
    sheet = til.reorder(api.PlasmaSheet(real, valid, ion), geom)
    sreal, svalid = sheet.numpy()
    if stale:   # move every 5th particle far away from its home tile without re-sorting
        rng = np.random.default_rng(1)
        idx = np.arange(0, sreal.shape[1], 5)
        sreal[0, idx] = rng.uniform(LO[0] + 0.01, HI[0] - 0.01, idx.size)
        sreal[1, idx] = rng.uniform(LO[1] + 0.01, HI[1] - 0.01, idx.size)
        sreal[6], sreal[7] = sreal[0], sreal[1]
    sion = np.zeros(sreal.shape[1], dtype=np.int32)
    slab = smooth_slab(n, n, g, amp=0.2)

    def fresh():
        return api.PlasmaSheet(sreal, svalid, sion), api.Fields(n, n, g, NCOMP, data=slab)

    # deposit
    ref = slab.copy()
    comp = [15, 16, -1, 18, 2, 17]
    oracle.deposit_current(ref, n, n, g, sreal.copy(), svalid.copy(), sion, ogeom, comp, -1.0, 1.0, order)
    pl, f = fresh()
    til.fallback.zero_()
    api.DepositCurrent(pl, f, geom, -1.0, 1.0, order, jx=15, jy=16, rho=18, chi=2, rhomjz=17, tiling=til)
    out = f.numpy()
    for c in (15, 16, 18, 2, 17):
        assert rel_err(out[c] - slab[c], ref[c] - slab[c]) < 1e-12, c
    assert (til.fallback.item() > 0) == stale

    # explicit deposit
    ref = slab.copy()
    oracle.explicit_deposit(ref, n, n, g, sreal.copy(), svalid.copy(), sion, ogeom, [10, 7, 5, 6], [3, 4], -1.0, 1.0, order, 2)
    pl, f = fresh()
    api.ExplicitDeposition(pl, f, geom, -1.0, 1.0, order, Bz=10, Ez=7, ExmBy=5, EypBx=6, Sy=3, Sx=4, tiling=til)
    out = f.numpy()
    for c in (3, 4):
        assert rel_err(out[c] - slab[c], ref[c] - slab[c]) < 1e-12, c

    # gather + push
    r2, v2 = sreal.copy(), svalid.copy()
    oracle.advance_plasma(slab, n, n, g, r2, v2, sion, ogeom, [11, 7, 8, 9, 10], -1.0, 1.0, order)
    pl, f = fresh()
    api.AdvancePlasmaParticles(pl, f, geom, -1.0, 1.0, order, Psi=11, Ez=7, Bx=8, By=9, Bz=10, tiling=til)
    greal, gvalid = pl.numpy()
    assert np.array_equal(gvalid, v2)
    live = v2 != 0
    for k in range(11):
        assert rel_err(greal[k][live], r2[k][live]) < 1e-10, k


@pytest.mark.parametrize("tile_size,period", [(0, 1), (16, 1), (16, 7), (32, 5)])
def test_engine_checksums_any_tiling(api, tile_size, period):
    """The reference pins particle re-ordering only through 'same checksums with
    plasmas.reorder_period = 4' (tests/blowout_wake_explicit.2Rank.sh:45-56); same bar here."""
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    deck = decks.blowout_wake()
    deck["n_steps"] = 1
    eng = api.SliceEngine(deck, tile_size=tile_size, sort_period=period)
    eng.set_diagnostics(True)
    eng.run_step()
    cs = eng.checksums()
    for k, v in gold.items():
        if v != 0.0:
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (k, cs[k], v)


def test_pipeline_driver_single_rank_on_gpu(api):
    """The ring driver with world_size 1 (in-process hand-off, MultiBuffer.cpp:299-308) on the GPU:
    the beam reaches step 1 only through the hand-off buffers."""
    import torch
    from hipace_amd.pipeline import run_pipeline
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    eng = api.SliceEngine(decks.blowout_wake())
    eng.set_diagnostics(True)
    sums = {}
    solved = run_pipeline(eng, 0, 1, 2, torch.device("cuda", 0), on_step_end=lambda s: sums.__setitem__(s, eng.checksums()))
    assert solved == 200 and set(sums) == {0, 1}
    for k, v in gold.items():
        if v != 0.0:
            assert abs(sums[1][k] - v) <= 1e-9 * abs(v), (k, sums[1][k], v)


# ------------------------------------------------------------------------------------------------
# moving driver beam: beam slice push, slipped-particle hand-off, several time steps
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_beam_evolution_matches_reference_checksums(api, oracle):
    """tests/beam_evolution.1Rank.sh: 21 steps of dt = 3 in a linear focusing field; field checksums of the last
    step against the reference's JSON (its CI: rtol 1e-12 on CPU, 2e-6 on GPU), beam state against the oracle."""
    deck = decks.beam_evolution()
    gold = json.load(open(os.path.join(GOLD, "beam_evolution.1Rank.json")))["lev=0"]
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_diagnostics(True)
    for _ in range(deck["n_steps"]):
        eng.run_step()
    cs = eng.checksums()
    for k, v in gold.items():
        if v == 0.0:
            assert cs[k] == 0.0, (k, cs[k])
        else:
            assert abs(cs[k] - v) <= 1e-9*abs(v), (k, cs[k], v)
    ref = oracle.Engine(deck)
    ref.run()
    bnd, soa = eng.beam_state()
    nz = deck["nz"]
    for p in range(nz):
        want = ref.beam_slice(nz - 1 - p)
        got = soa[:, bnd[p]:bnd[p + 1]]
        assert got.shape == want.shape                      # nobody slips in this deck
        assert np.abs(got - want).max() <= 1e-10*np.abs(want).max()


@pytest.mark.gpu
@pytest.mark.parametrize("dt,n_steps", [(0.9, 6), (4.0, 2)])
def test_beam_slipping_matches_oracle(api, oracle, dt, n_steps):
    """A slow, hot beam (u_z = 1.2: v_z = 0.77 c) falls back through the slices: the slice populations and every
    particle's state after the steps equal the oracle's (as sets: the device partition is not order preserving).
    dt = 4: a particle slips 0.23*4/0.4 = 2.3 cells per step, i.e. through SEVERAL slices in one step, and is pushed again
    on every slice it lands on (BeamParticleAdvance.cpp:131, "IncludingSlipped") -- slices that were empty at the start
    of the step fill up during it."""
    deck = decks.beam_evolution()
    deck.update(nz=12, lo=(-2.0, -2.0, -2.4), hi=(2.0, 2.0, 2.4), beam_zmin=-1.0, beam_zmax=1.6, beam_umean=(0.0, 0.0, 1.2),
                beam_density=1.0e-3, n_steps=n_steps, dt=dt, beam_n_subcycles=4 if dt < 1 else 16, ext_E_slope=(0.3, 0.2))
    if dt > 1:
        deck.update(beam_zmin=0.4, beam_zmax=1.6)        # three populated slices at the head, nine empty ones behind
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_diagnostics(True)
    for _ in range(deck["n_steps"]):
        eng.run_step()
    ref = oracle.Engine(deck)
    ref.run()
    bnd, soa = eng.beam_state()
    nz = deck["nz"]
    moved = 0
    n0 = oracle.Engine(deck)
    for p in range(nz):
        want = ref.beam_slice(nz - 1 - p)
        got = soa[:, bnd[p]:bnd[p + 1]]
        assert got.shape == want.shape, (p, got.shape, want.shape)
        moved += abs(want.shape[1] - n0.beam_slice(nz - 1 - p).shape[1])
        if want.shape[1]:
            ko = np.lexsort((want[1], want[0])); kg = np.lexsort((got[1], got[0]))
            assert np.abs(got[:, kg] - want[:, ko]).max() <= 1e-10*np.abs(want).max()
    assert moved > 0                                           # the deck does make particles slip
    cs, rs = eng.checksums(), ref.checksums()
    for k in ("jz_beam", "Bx", "By", "Ez", "Sx", "Sy"):
        assert abs(cs[k] - rs[k]) <= 1e-9*max(abs(rs[k]), 1e-300), (k, cs[k], rs[k])


@pytest.mark.gpu
def test_beam_push_with_radiation_reaction_matches_oracle(api, oracle):
    """<beam>.do_radiation_reaction and do_z_push = 0 (particles/pusher/BeamParticleAdvance.cpp:244-297, 316) on the deck of
    the oracle's theory test (examples/beam_in_vacuum/inputs_RR in normalised units): every particle's state after six
    steps equals the oracle's to 1e-10, and the energy lost is the oracle's."""
    deck = decks.radiation_reaction()
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_insitu_beam(float("inf"))
    for _ in range(deck["n_steps"]):
        eng.run_step()
    ref = oracle.Engine(deck)
    ref.set_insitu_beam(float("inf"))
    ref.run()
    bnd, soa = eng.beam_state()
    nz = deck["nz"]
    total = 0
    for p in range(nz):
        want = ref.beam_slice(nz - 1 - p)
        got = soa[:, bnd[p]:bnd[p + 1]]
        assert got.shape == want.shape, (p, got.shape, want.shape)
        total += want.shape[1]
        if want.shape[1]:
            # symmetric partners share |x|, |y| to rounding: order by rounded keys
            ko = np.lexsort((np.round(want[1], 6), np.round(want[0], 6))); kg = np.lexsort((np.round(got[1], 6), np.round(got[0], 6)))
            assert np.abs(got[:, kg] - want[:, ko]).max() <= 1e-10 * np.abs(want).max()
    assert total > 100
    gi, oi = eng.insitu_beam(), ref.insitu_beam()
    w = oi[0]
    g_ref = (w * oi[20]).sum() / w.sum()
    g_gpu = (gi["sum(w)"] * gi["[ga]"]).sum() / gi["sum(w)"].sum()
    assert 2000.0 - g_ref > 5.0 and abs(g_gpu - g_ref) < 1e-9 * g_ref
    # normalised units without hipace.background_density_SI: refused as the reference asserts (:39-43)
    with pytest.raises(RuntimeError):
        api.SliceEngine(dict(deck, background_density_SI=0.0))


@pytest.mark.gpu
def test_moving_beam_through_the_ring_hand_off(api, oracle):
    """world = 1 pipeline (in-process hand-off through export / import messages on the device) of a beam that slips
    every step: per-step checksums equal those of the oracle stepping the same deck."""
    import torch
    from hipace_amd.pipeline import run_pipeline
    deck = decks.beam_evolution()
    deck.update(nz=12, lo=(-2.0, -2.0, -2.4), hi=(2.0, 2.0, 2.4), beam_zmin=-1.0, beam_zmax=1.6, beam_umean=(0.0, 0.0, 1.2),
                beam_density=1.0e-3, n_steps=4, dt=0.9, beam_n_subcycles=4, ext_E_slope=(0.3, 0.2))
    ref = oracle.Engine(deck)
    want = {}
    for s in range(deck["n_steps"]):
        ref.begin_step()
        for k in range(deck["nz"] - 1, -1, -1):
            ref.solve_slice(k)
        want[s] = ref.checksums()
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_diagnostics(True)
    got = {}
    solved = run_pipeline(eng, 0, 1, deck["n_steps"], torch.device("cuda", 0), on_step_end=lambda s: got.__setitem__(s, eng.checksums()))
    assert solved == deck["n_steps"]*deck["nz"]
    for s in want:
        for k in ("jz_beam", "jx_beam", "Bx", "By", "Ez", "Sx", "Sy"):
            assert abs(got[s][k] - want[s][k]) <= 1e-9*max(abs(want[s][k]), 1e-300), (s, k, got[s][k], want[s][k])
    eng.beam_state()            # raises if a slice outgrew the message capacity


# ---- predictor-corrector Bx/By (BASELINE config 2 runs this solver) -------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tile_size", [0, 16])
@pytest.mark.parametrize("settings", [(1.0e-4, 7, 0.0635), (4.0e-2, 30, 0.05)])
def test_predictor_corrector_slice_by_slice_vs_oracle(api, oracle, tile_size, settings):
    """hipace.bxby_solver = predictor-corrector (Hipace.cpp:935-1031) against the oracle, whose loop is pinned on the
    reference's beam_in_vacuum_open_boundary checksums: every slab component and the particle sheet, slice by slice,
    with the loop settings of the reference's own test (ion_motion.SI.1Rank.sh) and with the code defaults."""
    from hipace_amd._lib import COMPS_PC
    base = decks.linear_wake_gaussian()
    # The beam reaches the first slice on purpose.  Where B is exactly zero the reference's error measure returns 0
    # (Fields.cpp:1283, norm_B > 0 ? ... : 0) and the loop stops after one pass; ahead of a beam the serial oracle has
    # exact zeros (electron and ion charge cancel term by term) where any atomic scatter leaves 1e-16 residue, so the
    # two would take different numbers of passes there (predictor-corrector).
    base.update(nz=60, lo=(-10.0, -10.0, -4.0), hi=(10.0, 10.0, 2.0), beam_zmin=-3.9, beam_zmax=2.5)
    deck = decks.predictor_corrector(base, *settings)
    ge = api.SliceEngine(deck, tile_size=tile_size, sort_period=5)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        if isl % 7 == 0:
            gs, os_ = ge.slab(), oe.slab()
            for c in range(ge.ncomp):
                assert rel_err(gs[c], os_[c]) < 1e-9, (isl, COMPS_PC[c], rel_err(gs[c], os_[c]))
    assert ge.pc_stats()[0] == oe.pc_stats()[0]                 # same number of iterations on every slice
    assert abs(ge.pc_stats()[1] - oe.pc_stats()[1]) <= 1e-9 * oe.pc_stats()[1]
    greal, gvalid = ge.particles()
    oreal, ovalid = oe.particles()
    if tile_size:
        gk = np.lexsort((np.round(greal[0], 7), np.round(greal[1], 7)))
        ok = np.lexsort((np.round(oreal[0], 7), np.round(oreal[1], 7)))
        greal, gvalid, oreal, ovalid = greal[:, gk], gvalid[gk], oreal[:, ok], ovalid[ok]
    assert np.array_equal(gvalid, ovalid)
    for k in range(11):
        assert rel_err(greal[k], oreal[k]) < 1e-9, k


@pytest.mark.gpu
def test_predictor_corrector_config2_head_slices(api, oracle):
    """BASELINE config 2: linear_wake.normalized on 256 x 256 x 512 at 4 ppc with the predictor-corrector solver --
    the first slices through the beam against the oracle (checksums over those slices).  Tolerance 1e-7: the wake has
    barely started (|ExmBy| ~ 1e-8 per cell) and sits that close to the 1e-16 residue the scatter's summation
    order leaves of the electron-ion charge cancellation."""
    deck = decks.predictor_corrector(decks.linear_wake(), 4.0e-2, 30, 0.05)
    deck.update(nx=256, ny=256, nz=512, plasma_ppc=(2, 2))
    ge = api.SliceEngine(deck, tile_size=16, sort_period=16)
    ge.set_diagnostics(True)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    # the slices ahead of the beam head (z = 1) are field-free: start on the first slice that holds beam particles
    # (the static beam blocks are addressed by slice, so both engines may start anywhere).  Two slices only: the
    # oracle's DST of length 257 (prime) costs about a second per loop iteration.
    first = 457
    assert ge.beam_layout()[1][512 - first] > 0 and ge.beam_layout()[1][512 - first - 1] == 0
    for isl in range(first, first - 2, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
    gc, oc = ge.checksums(), oe.checksums()
    for k, v in oc.items():
        if v == 0.0:
            assert gc[k] == 0.0, k
        else:
            assert abs(gc[k] - v) <= 1e-7 * abs(v), (k, gc[k], v)
    assert ge.pc_stats()[0] == oe.pc_stats()[0]


@pytest.mark.gpu
@pytest.mark.parametrize("solver,tile_size", [(0, 16), (0, 0), (1, 16)])
def test_open_field_boundary_slice_by_slice_vs_oracle(api, oracle, solver, tile_size):
    """boundary.field = Open (Fields::SetBoundaryCondition, fields/Fields.cpp:678-735: the sources' multipole moments to order
    18, their free-space potential one cell outside the box as Dirichlet values of Psi, Ez, Bz -- and of Bx, By inside the
    predictor-corrector loop): a wake whose fields reach the walls (the blowout deck in a box of half the width, the driver
    off centre) under both Bx/By solvers, every slab component every fifth slice and the checksums against the oracle, whose
    restatement is pinned on the reference's beam_in_vacuum_open_boundary file -- which the engine also reproduces itself
    (test_engine_reproduces_reference_checksums).  The open walls do change the answer: Psi at the wall is not 0."""
    from hipace_amd._lib import COMPS, COMPS_PC
    base = decks.blowout_wake()
    base.update(nz=40, n_steps=1, lo=(-4.0, -4.0, 1.2), hi=(4.0, 4.0, 6.0), beam_pos_mean=(0.6, -0.4, 0.0), field_bc=1)
    deck = decks.predictor_corrector(base, 1.0e-4, 7, 0.0635) if solver else base
    names = COMPS_PC if solver else COMPS
    ge = api.SliceEngine(deck, tile_size=tile_size, sort_period=5)
    ge.set_diagnostics(True)
    oe = oracle.Engine(deck)
    ce = api.SliceEngine(dict(deck, field_bc=0), tile_size=tile_size, sort_period=5)      # closed walls, for contrast
    ge.begin_step()
    oe.begin_step()
    ce.begin_step()
    wall = 0.0
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        ce.solve_slice(isl)
        if isl % 5 == 0:
            gs, os_, cs_ = ge.slab(), oe.slab(), ce.slab()
            for c in range(ge.ncomp):
                assert rel_err(gs[c], os_[c]) < 1e-9, (isl, names[c], rel_err(gs[c], os_[c]))
            g = (gs.shape[1] - deck["ny"]) // 2
            ipsi = list(names).index("Psi")
            wall = max(wall, np.abs(gs[ipsi][g, g:-g]).max() / np.abs(gs[ipsi]).max())
            assert rel_err(gs[ipsi], cs_[ipsi]) > 1e-3
    assert wall > 1e-3, wall
    gc, oc = ge.checksums(), oe.checksums()
    for k, v in oc.items():
        if v:
            assert abs(gc[k] - v) <= 1e-9 * abs(v), (k, gc[k], v)
    if solver:
        assert ge.pc_stats()[0] == oe.pc_stats()[0]
    else:
        assert ge.stats()["vcycles"] == oe.vcycles()


@pytest.mark.gpu
def test_open_field_boundary_serial_and_pipelined(api):
    """open walls with three time steps in flight on the device (every engine has its own moments buffer and staging planes):
    the checksums of every step equal the serial run's"""
    import torch
    from hipace_amd.pipeline import run_lanes
    deck = dict(decks.blowout_wake(), nz=40, lo=(-4.0, -4.0, 1.2), hi=(4.0, 4.0, 6.0), beam_pos_mean=(0.6, -0.4, 0.0), field_bc=1, n_steps=4)

    def engine():
        e = api.SliceEngine(deck, tile_size=16)
        e.set_diagnostics(True)
        return e

    ser = engine()
    want = []
    for _ in range(4):
        ser.run_step()
        want.append(ser.checksums())
    got = {}
    run_lanes([engine() for _ in range(3)], 0, 1, 4, torch.device("cuda", 0), on_step_end=lambda step, e: got.__setitem__(step, e.checksums()))
    assert sorted(got) == [0, 1, 2, 3]
    for step in range(4):
        for k, v in want[step].items():
            assert abs(got[step][k] - v) <= 1e-10 * abs(v), (step, k, got[step][k], v)


# ---- beam particles -> slices (integer work: bit-exact) ---------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,num_boxes", [(0, 8), (1, 1), (1000, 7), (200000, 1024), (65537, 100)])
def test_beam_sort_by_box_bit_exact(api, oracle, n, num_boxes):
    """BoxSorter::sortParticlesByBox against the oracle's restatement of the serial CPU result: counts, offsets and
    permutation equal bit for bit, including particles below / above the box (-> the extra last box), particles
    exactly on box edges, an empty beam and a single box."""
    import torch
    rng = np.random.default_rng(n + num_boxes)
    plo, dz = -3.0, 6.0 / num_boxes
    z = rng.uniform(-3.6, 3.6, n)
    if n >= 1000:
        z[:50] = plo + dz * rng.integers(0, num_boxes + 1, 50)      # exactly on edges
        z[50:60] = plo - 0.3 * dz                                   # truncation toward zero keeps these in box 0
        z[60:70] = plo - 1.0 * dz
    want = oracle.beam_sort_by_box(z, plo, dz, num_boxes)
    got = api.BoxSorter().sortParticlesByBox(torch.as_tensor(z, device="cuda"), plo, dz, num_boxes)
    assert np.array_equal(got.boxCounts, want[0])
    assert np.array_equal(got.boxOffsets, want[1])
    assert np.array_equal(got.boxPermutations, want[2])
    assert int(got.boxCounts.sum()) == n


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,n_steps", [(2, 3), (3, 5)])
def test_several_steps_in_flight_on_one_gpu(api, lanes, n_steps):
    """pipeline.run_local_pipeline on the GPU: `lanes` engines on their own streams, coupled by events and the
    per-slice beam copy, reproduce the reference's blowout_wake checksums on every step."""
    import torch
    from hipace_amd.pipeline import run_local_pipeline
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    deck = decks.blowout_wake()
    deck["n_steps"] = 1
    engs = [api.SliceEngine(deck, tile_size=16, sort_period=16) for _ in range(lanes)]
    for e in engs:
        e.set_diagnostics(True)
    got = {}

    def on_step_end(step, eng):
        eng.sync()
        got[step] = eng.checksums()

    solved = run_local_pipeline(engs, n_steps, torch.device("cuda", 0), on_step_end)
    assert solved == n_steps * deck["nz"] and sorted(got) == list(range(n_steps))
    for step, cs in got.items():
        for k, v in gold.items():
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (step, k, cs[k], v)


@pytest.mark.gpu
@pytest.mark.parametrize("edge", ["rccl", "ipc"])
@pytest.mark.parametrize("lanes,n_steps", [(2, 5), (3, 7)])
def test_several_stages_per_rank_with_the_closing_edge_on_rccl(api, lanes, n_steps, edge):
    """What a rank of a multi-rank ring with several stages does, on the one rank a 1-GPU box has: `lanes` engines are the
    stages of this process, the edges between them are in-process copies, and the edge that closes the ring -- last stage
    -> first stage -- goes through RCCL (RcclSelfRing: ncclSend + ncclRecv on the ring's streams, the first stage's
    receives posted a step ahead, ordered against the engines by events only).  Every step has the reference's checksums."""
    import torch
    from hipace_amd.pipeline import RcclSelfRing, run_lanes
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    deck = decks.blowout_wake()
    deck["n_steps"] = 1
    engs = [api.SliceEngine(deck, tile_size=16, sort_period=16) for _ in range(lanes)]
    for e in engs:
        e.set_diagnostics(True)
    got = {}

    def on_step_end(step, eng):
        eng.sync()
        got[step] = eng.checksums()

    T = RcclSelfRing(0, edge=edge)          # (ipc with one rank: the ring's streams and events, a device copy as the message)
    assert T.kind == edge
    solved = run_lanes(engs, 0, 1, n_steps, torch.device("cuda", 0), on_step_end, transport=T)
    st = T.stats()
    T.close()
    assert solved == n_steps * deck["nz"] and sorted(got) == list(range(n_steps))
    assert st["sent"] > 0 and st["sent"] == st["received"]                # the closing edge's messages went through RCCL
    for step, cs in got.items():
        for k, v in gold.items():
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (step, k, cs[k], v)


# ---- field diagnostics (Fields::Copy into the 3-D output array) ------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("coarsening", [(1, 1, 1), (3, 4, 5), (2, 2, 2)])
def test_field_diagnostic_matches_oracle(api, oracle, coarsening):
    """hps_engine_set_field_diagnostic / field_diagnostic against the oracle's restatement of Fields::Copy (itself
    pinned by the reference's analysis_coarsening criterion): 60 x 60 x 100 blowout deck, the fields the reference's
    coarsening test writes, <= 1e-9 of each field's maximum; coarsening 1 1 1 also reproduces the checksums."""
    deck = decks.blowout_wake()
    deck.update(nx=60, ny=60, nz=100, n_steps=1)
    names = ["Ez", "ExmBy", "EypBx", "Bx", "By", "Bz"]
    ge = api.SliceEngine(deck, tile_size=16, sort_period=16)
    ge.set_diagnostics(True)
    ge.set_field_diagnostic(names, coarsening)
    oe = oracle.Engine(deck)
    od = oracle.FieldDiagnostic(deck, [oracle.CIDX[n] for n in names], coarsening)
    ge.begin_step()
    oe.begin_step()
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        od.add_slice(isl, oe.slab(), oe.g)
    got = ge.field_diagnostic()
    for n, name in enumerate(names):
        assert got[name].shape == od.F[n].shape
        assert np.abs(got[name] - od.F[n]).max() <= 1e-9 * np.abs(od.F[n]).max(), name
    if coarsening == (1, 1, 1):
        cs = ge.checksums()
        for name in names:
            assert abs(np.abs(got[name]).sum() - cs[name]) <= 1e-12 * cs[name]
    # a second step starts from a cleared array
    ge.begin_step()
    assert all(np.all(v == 0.0) for v in ge.field_diagnostic().values())


@pytest.mark.gpu
def test_insitu_field_reductions_match_oracle(api, oracle):
    """Fields::InSituComputeDiags: the ten per-slice reductions of every slice of the blowout_wake deck against the
    oracle's restatement on its own slab (<= 1e-10 of each quantity's largest slice value)."""
    deck = decks.blowout_wake()
    deck["n_steps"] = 1
    ge = api.SliceEngine(deck, tile_size=16, sort_period=16)
    ge.set_insitu_fields(True)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    want = np.zeros((10, deck["nz"]))
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        # jz_beam of this slice is still in place after the push (ShiftSlices moves jx/jy only)
        want[:, isl] = oracle.insitu_fields(oe.slab(), oe.g, deck)
    got = ge.insitu_fields()
    for q, name in enumerate(api.SliceEngine.INSITU_FIELDS):
        scale = np.abs(want[q]).max()
        assert scale > 0 and np.abs(got[name] - want[q]).max() <= 1e-10 * scale, name


# ---- error behaviour: status + message instead of the reference's amrex::Abort ------------------------------------
@pytest.mark.gpu
def test_error_behaviour(api):
    """Where the reference aborts the process (AMREX_ALWAYS_ASSERT / amrex::Abort), the C ABI returns a status and
    hps_last_error() names the call; the Python mirror raises HpsError (a RuntimeError).  Nothing is computed."""
    import torch
    from hipace_amd import _lib
    g = G2

    def fails(fn, needle):
        with pytest.raises(RuntimeError) as ei:
            fn()
        assert needle in str(ei.value), str(ei.value)

    # solver / slab size mismatch, bad component (HpMultiGrid.H:168-175 center_box asserts; Fields getField)
    f = api.Fields(64, 64, g, 6)
    ps = api.FFTPoissonSolver(32, 32, 0.1, 0.1)
    fails(lambda: ps.SolvePoissonEquation(f, 1), "does not match")
    fails(lambda: api.FFTPoissonSolver(64, 64, 0.1, 0.1).SolvePoissonEquation(f, 9), "component")
    mg = api.MultiGrid(32, 32, 0.1, 0.1)
    fails(lambda: mg.solve1(f, 0, 2, 4), "does not match")
    fails(lambda: api.MultiGrid(64, 64, 0.1, 0.1).solve1(f, 5, 2, 4), "component")      # sol needs 2 adjacent comps
    # hpmg aborts when nummaxiter V-cycles do not reach the tolerance (HpMultiGrid.cpp:1409-1416)
    f.t[2:4, g:-g, g:-g] = torch.randn((2, 64, 64), dtype=torch.float64, device="cuda")
    f.t[4] = 1.0
    fails(lambda: api.MultiGrid(64, 64, 0.1, 0.1).solve1(f, 0, 2, 4, tol_rel=1e-14, nummaxiter=1), "not converged")
    # deposition order, tile size, guard cells
    fails(lambda: api.Tiling(64, 64, 24, 100), "tile_size")
    deck = decks.blowout_wake()
    fails(lambda: api.SliceEngine(dict(deck, order=4)), "depos_order")
    fails(lambda: api.SliceEngine(dict(deck, field_bc=2)), "boundary.field")
    fails(lambda: api.SliceEngine(dict(deck, field_bc=1, lo=(1.0, -8.0, -6.0), hi=(17.0, 8.0, 6.0))), "inside the box")   # open walls expand about x = y = 0
    # engine options that do not apply
    eng = api.SliceEngine(deck)
    fails(lambda: eng.set_field_diagnostic(["Ez"], (3, 1, 1)), "divisible")             # 64 % 3 != 0
    pc = api.SliceEngine(decks.predictor_corrector(deck))
    fails(lambda: pc.set_insitu_fields(True), "explicit solver only")
    mv = api.SliceEngine(decks.beam_evolution())
    buf = torch.zeros(7 * max(mv.beam_layout()[0], 1), dtype=torch.float64, device="cuda")
    fails(lambda: mv.set_beam_storage(buf), "dt")
    assert isinstance(_lib.lib().hps_last_error(), bytes)


@pytest.mark.gpu
def test_insitu_plasma_moments_match_oracle(api, oracle):
    """PlasmaParticleContainer::InSituComputeDiags: the 15 per-slice entries (taken before the slice is solved, within
    a radius of 4) against the oracle's restatement on its own particle sheet."""
    deck = decks.blowout_wake()
    deck.update(nz=40, n_steps=1)
    ge = api.SliceEngine(deck, tile_size=16, sort_period=8)
    ge.set_insitu_plasma(4.0)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    want = np.zeros((15, deck["nz"]))
    for isl in range(deck["nz"] - 1, -1, -1):
        oreal, ovalid = oe.particles()
        want[:, isl] = oracle.insitu_plasma(oreal, ovalid, 4.0)
        ge.solve_slice(isl)
        oe.solve_slice(isl)
    got = ge.insitu_plasma()
    assert np.array_equal(got["Np"], want[14])                       # particle counts: exact
    for q, name in enumerate(api.SliceEngine.INSITU_PLASMA[:14]):
        scale = max(np.abs(want[q]).max(), 1e-300)
        # first moments of a symmetric sheet are pure cancellation: compare against the second moments' scale
        ref = max(scale, np.sqrt(np.abs(want[min(q + 1, 13)]).max()) if name in ("[x]", "[y]", "[ux]", "[uy]") else scale)
        assert np.abs(got[name] - want[q]).max() <= 1e-9 * ref, name


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["static", "moving"])
def test_insitu_beam_moments_match_oracle(api, oracle, case):
    """BeamParticleContainer::InSituComputeDiags: the 23 per-slice entries (after the field solves, before the beam
    push; particles that slipped in from the slice ahead are not counted) against the oracle.  static: the blowout deck
    (dt = 0, within a radius of 0.5); moving: four steps of the beam_evolution deck with a time step large enough for
    particles to slip."""
    if case == "static":
        deck = decks.blowout_wake()
        deck.update(nz=40, n_steps=1)
        radius = 0.5
    else:
        deck = decks.beam_evolution()
        deck.update(n_steps=4, dt=30.0, beam_umean=(0.0, 0.0, 20.0))
        radius = float("inf")
    ge = api.SliceEngine(deck, tile_size=16, sort_period=8)
    oe = oracle.Engine(deck)
    ge.set_insitu_beam(radius)
    oe.set_insitu_beam(radius)
    for _ in range(deck["n_steps"]):
        ge.run_step()
        oe.begin_step()
        for isl in range(deck["nz"] - 1, -1, -1):
            oe.solve_slice(isl)
    got, want = ge.insitu_beam(), oe.insitu_beam()
    assert want[22].sum() > 0 and np.array_equal(got["Np"], want[22])           # particle counts: exact
    if case == "moving":
        assert want[22].sum() < oe.beam_layout()[0]                                # some have slipped or left
    for q, name in enumerate(api.SliceEngine.INSITU_BEAM[:22]):
        scale = max(np.abs(want[q]).max(), 1e-300)
        # first moments of a symmetric beam are pure cancellation: compare against the second moments' scale
        if name in ("[x]", "[y]", "[ux]", "[uy]"):
            scale = max(scale, np.sqrt(np.abs(want[q + 1]).max()))
        elif name in ("[x*ux]", "[y*uy]", "[x*uy]", "[y*ux]", "[ux/uz]", "[uy/uz]"):
            scale = max(scale, np.sqrt(np.abs(want[2]).max() * np.abs(want[8]).max()), 1e-12)
        assert np.abs(got[name] - want[q]).max() <= 1e-9 * scale, (name, np.abs(got[name] - want[q]).max(), scale)


@pytest.mark.gpu
def test_bench_line_contract():
    """bench.py prints one JSON line with the agreed keys (a short run: 96 timed slices of the headline workload)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "96", "--warmup", "8",
                          "--cpu-slices", "1"], capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 96 and d["warmup"] == 8 and d["unit"] == "slices/s"
    assert d["dtype"] == "f64" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["higher_is_better"] is True
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0.05 < r["frac"] < 1.0
    assert r["traffic"] is None or r["traffic"] >= 0.9 * r["algorithmic_bytes_per_launch"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and 1 <= c["cores"] <= c["host_cores"] and c["unit"] == "slices/s" and c["value"] > 0
    assert c["serial_value"] > 0
    assert "workload" in d["config"] and "model" not in d["config"]
    # a short run is not taken at the (cheap) head of the box, every 16th timed slice carries the event timers (every 2nd of
    # fewer than 64), and the line says where the traffic figure comes from
    t = d["timed_slices"]
    assert t["first"] >= 400 and t["last"] - t["first"] + 1 == 96 and 5 <= d["profiled_slices"] <= 7
    sl = r["slice"]
    assert sl["algorithmic_bytes_fused_lower_bound"] < sl["reference_passes"]["algorithmic_bytes"] and 0.15 < sl["frac_fused_lower_bound"] < 1.0
    assert sl["counter_bytes_per_slice"] is None or (sl["counter_bytes_per_slice"] > 0.8 * sl["algorithmic_bytes_fused_lower_bound"]
                                                     and abs(sl["frac_counter_bytes"] - sl["achieved_counter"] / r["peak"]) < 1e-12)
    fl = d["in_flight"]
    assert fl is None or 0.15 < fl["roofline"]["frac_fused_lower_bound"] < 1.0
    assert r["traffic"] is None or "profiles/" in r["traffic_source"]
    assert d["vcycles_per_slice"] > 1.0


@pytest.mark.gpu
def test_bench_short_run_times_every_slice():
    """The driver's `--steps 20 --warmup 5`: 20 slices at the representative window, the four event records of the roofline's
    kernel duration on every second one of them (on every one they cost 0.9 % of the rate)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                          "--cpu-slices", "0"], capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1])
    assert d["steps"] == 20 and d["warmup"] == 5 and d["profiled_slices"] == 10
    assert d["timed_slices"]["first"] >= 400 and d["vcycles_per_slice"] > 1.0


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_for_the_same_arguments(tmp_path):
    """--dump-outputs DIR: the last timed slice's fields and plasma particles as float64 .npy files, a seeded sample
    of the large ones (64 MB at most); two runs with the same arguments compute the same values (atomics: to 1e-12)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                              "--n", "128", "--cpu-slices", "0", "--inflight", "1", "--phase-window", "0", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        assert json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1])["steps"] == 6
        dumps.append({p.name: np.load(p) for p in sorted(d.iterdir())})
    a, b = dumps
    assert sorted(a) == sorted(b) and "field_Psi.npy" in a and "plasma_x.npy" in a
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and a[name].shape == b[name].shape and a[name].size > 0, name
        assert np.abs(a[name] - b[name]).max() <= 1e-12 * max(np.abs(b[name]).max(), 1e-300), name


@pytest.mark.gpu
def test_rccl_ring_carries_the_beam_on_one_gpu(api):
    """The C-ABI ring on RCCL with the one rank a 1-GPU box has: hps_ring_init makes a 1-rank communicator and
    hps_ring_sendrecv_self (MultiBuffer.cpp:299-308, "send to myself") moves every beam block of step 0 into the storage
    step 1 reads -- ncclSend / ncclRecv, ordered against the engine by events only.  Step 1 reproduces the reference's
    checksums, i.e. the beam did arrive through RCCL."""
    import torch
    from hipace_amd.pipeline import RcclTransport
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    deck = decks.blowout_wake()
    nz = deck["nz"]
    eng = api.SliceEngine(deck)
    eng.set_diagnostics(True)
    T = RcclTransport(0, 1, 0)
    nbeam, off = eng.beam_layout()
    bufs = [torch.zeros(7 * nbeam, dtype=torch.float64, device="cuda") for _ in range(2)]
    eng.initial_beam_into(bufs[0])
    moved = 0
    landed = {}
    eng.set_beam_storage(bufs[0], injected_beam_support=True)
    eng.begin_step()
    for q in range(nz):
        eng.solve_slice(nz - 1 - q)
        if off[q + 1] > off[q]:
            ev = eng.record_event(q % 64)                  # behind the slice's last kernel
            src, dst = bufs[0][7 * off[q]:7 * off[q + 1]], bufs[1][7 * off[q]:7 * off[q + 1]]
            landed[q] = T.sendrecv_self(src, dst, ev, q)   # ncclSend + ncclRecv as one group on the ring's stream
            moved += src.numel() * 8
    eng.set_beam_storage(bufs[1], injected_beam_support=True)
    eng.begin_step()
    for q in range(nz):
        for j in (q, q + 1):
            if j in landed:
                eng.wait_event(landed.pop(j))              # device-side: the block has landed
        eng.solve_slice(nz - 1 - q)
    eng.sync()
    T.finish()
    st = T.stats()
    assert st["sent"] == st["received"] > 0 and st["bytes_sent"] == moved == 7 * 8 * nbeam
    assert torch.equal(bufs[0], bufs[1])
    cs = eng.checksums()
    for k, v in gold.items():
        if v != 0.0:
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (k, cs[k], v)
    T.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["order1", "order3", "order0_absorbing", "nonsquare_reflecting", "fine_z_2ppc"])
def test_engine_variants_vs_oracle(api, oracle, case):
    """The slice loop away from the golden decks' settings: other deposition orders, particle boundaries, a
    non-square box whose sizes have no built DST factorisation (dense back-end in x and y), several particles per
    cell -- every slab component against the oracle after 30 slices, and the V-cycle counts."""
    from hipace_amd._lib import COMPS
    deck = decks.blowout_wake()
    # the beam reaches the first slice: on field-free slices the multigrid's "converged on entry" test compares
    # rounding noise (exact zeros in the serial oracle) and the V-cycle counts need not agree
    deck.update(nz=30, n_steps=1, lo=(-8.0, -8.0, -1.8), hi=(8.0, 8.0, 1.8), beam_zmin=-1.7, beam_zmax=2.5)
    if case == "order1":
        deck.update(order=1)
    elif case == "order3":
        deck.update(order=3)
    elif case == "order0_absorbing":
        deck.update(order=0, bc=2)
    elif case == "nonsquare_reflecting":
        deck.update(nx=48, ny=80, bc=0, lo=(-6.0, -10.0, -1.8), hi=(6.0, 10.0, 1.8))
    else:
        deck.update(plasma_ppc=(2, 2), nz=60)
    ge = api.SliceEngine(deck, tile_size=16, sort_period=6)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
    gs, os_ = ge.slab(), oe.slab()
    assert np.abs(os_[COMPS.index("Bx")]).max() > 1e-3
    for c in range(ge.ncomp):
        assert rel_err(gs[c], os_[c]) < 1e-9, (case, COMPS[c], rel_err(gs[c], os_[c]))
    assert ge.stats()["vcycles"] == oe.vcycles()
    greal, gvalid = ge.particles()
    oreal, ovalid = oe.particles()
    assert int(gvalid.sum()) == int(ovalid.sum())              # absorbed / dropped particles: same count


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["explicit", "predictor-corrector"])
def test_grid_current_drives_a_plasma_wake_vs_oracle(api, oracle, solver):
    """grid_current.* (utils/GridCurrent.cpp:25-71) on a plasma, no beam: the Gaussian current on the grid is the only
    driver; it goes into jz_beam (explicit solver) or jz (predictor-corrector).  Every slab component vs the oracle."""
    deck = decks.blowout_wake()
    deck.update(nz=24, n_steps=1, lo=(-8.0, -8.0, -1.8), hi=(8.0, 8.0, 1.8), beam_profile=-1,
                grid_current_on=1, grid_current_peak=-0.5, grid_current_mean=(0.5, -0.25, 2.0), grid_current_std=(0.6, 0.4, 1.0))
    if solver != "explicit":
        deck = decks.predictor_corrector(deck, tol=1e-3, max_iter=5, mix=0.05)
    ge = api.SliceEngine(deck, tile_size=16, sort_period=6)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
    gs, os_ = ge.slab(), oe.slab()
    names = ge.comp_names()
    assert np.abs(os_[names.index("Bx")]).max() > 1e-3
    for c in range(ge.ncomp):
        assert rel_err(gs[c], os_[c]) < 1e-9, (solver, names[c], rel_err(gs[c], os_[c]))
    if solver == "explicit":
        assert ge.stats()["vcycles"] == oe.vcycles()
    else:
        assert ge.pc_stats()[0] == oe.pc_stats()[0]


# ---- laser-driven wake (first half: static Gaussian envelope) ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tile_size", [0, 16])
def test_laser_blowout_wake_matches_reference_checksums(api, tile_size):
    """tests/laser_blowout_wake_explicit.1Rank.sh: no beam, a Gaussian laser pulse (a0 = 4.5) drives the wake through
    |a|^2 in the deposition, the explicit source and the pusher -- all 18 checksums of the reference's fixture
    (the reference skips Sx, Sy, chi; they agree too), incl. aabs and laserEnvelope."""
    gold = json.load(open(os.path.join(GOLD, "laser_blowout_wake_explicit.1Rank.json")))["lev=0"]
    eng = api.SliceEngine(decks.laser_blowout_wake(), tile_size=tile_size, sort_period=8)
    eng.set_diagnostics(True)
    eng.run_step()
    cs = eng.checksums()
    for k, v in gold.items():
        if v == 0.0:
            assert cs[k] == 0.0, k
        else:
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (k, cs[k], v)


@pytest.mark.gpu
def test_laser_wake_slice_by_slice_vs_oracle(api, oracle):
    deck = decks.laser_blowout_wake()
    deck.update(nx=64, ny=64, nz=40, lo=(-16.0, -16.0, -3.0), hi=(16.0, 16.0, 3.0), laser_pos=(1.0, -0.5, 0.5), order=3)
    ge = api.SliceEngine(deck, tile_size=16, sort_period=5)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    names = ge.comp_names()
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        if isl % 9 == 0:
            gs, os_ = ge.slab(), oe.slab()
            for c in range(ge.ncomp):
                assert rel_err(gs[c], os_[c]) < 1e-9, (isl, names[c], rel_err(gs[c], os_[c]))


@pytest.mark.gpu
def test_laser_evolution_fft_solver_matches_reference_checksums(api):
    """tests/laser_evolution.SI.2Rank.sh (lasers.solver_type = fft) on the GPU: 30 steps of the envelope solver in
    vacuum, then the checksums of the xz diagnostic slice (mean of the two central rows) as in the fixture."""
    gold = json.load(open(os.path.join(GOLD, "laser_evolution.SI.2Rank.json")))["lev=0"]
    deck = decks.laser_evolution()
    eng = api.SliceEngine(deck)
    for step in range(deck["n_steps"]):
        eng.run_step()
    a = eng.laser_envelope()
    ny = deck["ny"]
    env = np.abs(0.5 * (a[:, ny // 2 - 1, :] + a[:, ny // 2, :])).sum()
    aabs = np.abs(a) ** 2
    aabs_xz = (0.5 * (aabs[:, ny // 2 - 1, :] + aabs[:, ny // 2, :])).sum()
    assert abs(env - gold["laserEnvelope"]) <= 1e-9 * gold["laserEnvelope"], (env, gold["laserEnvelope"])
    assert abs(aabs_xz - gold["aabs"]) <= 1e-9 * gold["aabs"], (aabs_xz, gold["aabs"])


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("nx,ny", [(96, 64), (320, 224), (48, 40), (1024, 1024)])
def test_multigrid2_solve2_vs_oracle(api, oracle, warm, nx, ny):
    """hps_mg2_solve2 (hpmg system type 2: complex coefficient, Re an array, Im a scalar) against the oracle: same number
    of V-cycles, solution to 1e-10, from a zero and from a non-zero initial guess.  96 x 64: one LDS-tiled level;
    320 x 224: three of them with ragged tile edges; 48 x 40: single-workgroup levels only; 1024 x 1024: BASELINE config 5's size."""
    import torch
    rng = np.random.default_rng(11)
    dx, dy = 0.11, 0.13
    rhs = rng.standard_normal((2, ny, nx))
    ar = 3.0 + rng.random((ny, nx))
    ai = -7.5
    sol = 0.02 * rng.standard_normal((2, ny, nx)) if warm else np.zeros((2, ny, nx))
    want = sol.copy()
    it_ref, rn_ref = oracle.mg_solve2(want, rhs, ar, ai, dx, dy, tol_rel=1e-6)
    assert it_ref >= 2
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda").contiguous()
    tsol, trhs, tar, tai = t(sol), t(rhs), t(ar), t(np.array([ai]))
    it, rn = api.MultiGrid2(nx, ny, dx, dy).solve2(tsol, trhs, tar, tai, tol_rel=1e-6)
    assert it == it_ref
    assert rel_err(tsol.cpu().numpy(), want) < 1e-10
    assert abs(rn - rn_ref) <= 1e-6 * rn_ref
    # the equation itself: -(ar + i ai) phi + Lap(phi) = rhs at an interior point, to the solver's tolerance
    ph = want[0] + 1j * want[1]
    j, i = 20, 30
    lap = (ph[j, i - 1] + ph[j, i + 1] - 2 * ph[j, i]) / dx ** 2 + (ph[j - 1, i] + ph[j + 1, i] - 2 * ph[j, i]) / dy ** 2
    assert abs(lap - (ar[j, i] + 1j * ai) * ph[j, i] - (rhs[0, j, i] + 1j * rhs[1, j, i])) < 1e-4 * np.abs(rhs).max()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [1, 2])
def test_evolving_laser_in_plasma_vs_oracle(api, oracle, solver):
    """Laser pulse in a plasma, envelope advanced with the plasma's chi by the FFT solver (1, AdvanceSliceFFT) or the
    multigrid solver (2, AdvanceSliceMG = hpmg system type 2, initial guess = the previous slice's solution): three steps,
    the envelope array and every slab component of the last slice against the oracle; multigrid: same V-cycle count."""
    deck = decks.laser_blowout_wake()
    deck.update(nx=64, ny=64, nz=30, lo=(-16.0, -16.0, -4.0), hi=(16.0, 16.0, 4.0), laser_a0=1.5, laser_lambda0=0.4,
                laser_solver=solver, dt=5.0, n_steps=3)
    ge = api.SliceEngine(deck, tile_size=16, sort_period=7)
    oe = oracle.Engine(deck)
    first = None
    for step in range(3):
        ge.begin_step()
        oe.begin_step()
        for isl in range(deck["nz"] - 1, -1, -1):
            ge.solve_slice(isl)
            oe.solve_slice(isl)
        ga, oa = ge.laser_envelope(), oe.laser_envelope()
        assert np.abs(ga - oa).max() <= 1e-9 * np.abs(oa).max(), step
        first = oa.copy() if first is None else first
    assert np.abs(oa - first).max() > 1e-2 * np.abs(first).max()          # the pulse did evolve
    assert ge.laser_vcycles() == oe.laser_vcycles() and (ge.laser_vcycles() > 0) == (solver == 2)
    gs, os_ = ge.slab(), oe.slab()
    names = ge.comp_names()
    for c in range(ge.ncomp):
        assert rel_err(gs[c], os_[c]) < 1e-8, (names[c], rel_err(gs[c], os_[c]))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [2, 3])
def test_laser_envelope_through_steps_in_flight_on_one_gpu(api, lanes):
    """run_local_pipeline with an evolving laser pulse: the stages hand a_{n+1}, a_n on slice by slice on the device;
    five steps give the envelope of one engine running them in turn."""
    import torch
    from hipace_amd.pipeline import run_local_pipeline
    d = decks.laser_blowout_wake()
    d.update(nx=64, ny=64, nz=24, lo=(-16.0, -16.0, -4.0), hi=(16.0, 16.0, 4.0), laser_a0=1.5, laser_lambda0=0.4,
             laser_solver=1, dt=5.0)
    ref = api.SliceEngine(d, tile_size=16, sort_period=8)
    want = {}
    for s in range(5):
        ref.run_step()
        want[s] = ref.laser_envelope()
    engs = [api.SliceEngine(d, tile_size=16, sort_period=8) for _ in range(lanes)]
    got = {}

    def on_step_end(step, eng):
        got[step] = eng.laser_envelope()

    run_local_pipeline(engs, 5, torch.device("cuda", 0), on_step_end)
    for s in range(5):
        assert np.abs(got[s] - want[s]).max() <= 1e-10 * np.abs(want[s]).max(), s


@pytest.mark.gpu
def test_laser_slice_messages_round_trip(api):
    """hps_engine_export_laser_slice / import_laser_slice (the device-side pack / unpack of the envelope's hand-off,
    MultiBuffer.cpp:840-852, 913-925): what engine A passes on after a step is what engine B starts its next step from."""
    import torch
    d = decks.laser_blowout_wake()
    d.update(nx=64, ny=64, nz=12, lo=(-16.0, -16.0, -3.0), hi=(16.0, 16.0, 3.0), laser_a0=1.5, laser_lambda0=0.4,
             laser_solver=1, dt=5.0)
    a = api.SliceEngine(d)
    ref = api.SliceEngine(d)
    a.run_step()
    ref.run_step()
    ref.run_step()                       # the reference engine runs step 1 itself
    b = api.SliceEngine(d)
    b.set_laser_import(True, 1)
    b.begin_step()
    msg = torch.zeros(a.laser_message_doubles(), dtype=torch.float64, device="cuda")
    for isl in range(d["nz"] - 1, -1, -1):
        a.export_laser_slice(isl, msg)
        a.sync()
        b.import_laser_slice(isl, msg)
        b.sync()
    for isl in range(d["nz"] - 1, -1, -1):
        b.solve_slice(isl)
    assert np.abs(b.laser_envelope() - ref.laser_envelope()).max() <= 1e-12 * np.abs(ref.laser_envelope()).max()
    # and the step after that agrees too (a_{n-1} arrived as well)
    c = api.SliceEngine(d)
    c.set_laser_import(True, 2)
    c.begin_step()
    for isl in range(d["nz"] - 1, -1, -1):
        b.export_laser_slice(isl, msg)
        b.sync()
        c.import_laser_slice(isl, msg)
        c.sync()
    for isl in range(d["nz"] - 1, -1, -1):
        c.solve_slice(isl)
    ref.run_step()
    assert np.abs(c.laser_envelope() - ref.laser_envelope()).max() <= 1e-10 * np.abs(ref.laser_envelope()).max()


@pytest.mark.gpu
@pytest.mark.parametrize("tile_size", [0, 16])
def test_laser_blowout_wake_SI_matches_reference_checksums(api, tile_size):
    """tests/laser_blowout_wake_explicit.SI.1Rank.sh: the laser-driven wake in SI units (hipace.normalized_units = 0;
    the deck of BASELINE config 5 at test size) -- all 18 checksums of the reference's fixture."""
    gold = json.load(open(os.path.join(GOLD, "laser_blowout_wake_explicit.SI.1Rank.json")))["lev=0"]
    eng = api.SliceEngine(decks.laser_blowout_wake_SI(), tile_size=tile_size, sort_period=8)
    eng.set_diagnostics(True)
    eng.run_step()
    cs = eng.checksums()
    for k, v in gold.items():
        if v == 0.0:
            assert cs[k] == 0.0, k
        else:
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (k, cs[k], v)


# ---- ADK field ionisation: species "ion" + released electrons (BASELINE config 5) -----------------------
def _compare_ion_run(api, oracle, deck, tile_size, n_steps, tol=1e-8):
    """GPU engine against the oracle, step by step: same key -> the same draw for every ion whatever the tile sort did
    to its position in the sheet, so the same ions ionise on the same slices; fields, ion levels (matched by lattice
    index) and the set of released electrons agree."""
    ge = api.SliceEngine(deck, tile_size=tile_size)
    ge.set_diagnostics(True)
    oe = oracle.Engine(deck)
    nz = deck["nz"]
    total = 0
    for step in range(n_steps):
        ge.begin_step()
        oe.begin_step()
        for k in range(nz - 1, -1, -1):
            ge.solve_slice(k)
            oe.solve_slice(k)
        gs, os_ = ge.slab(), oe.slab()
        for c, name in enumerate(ge.comp_names()):
            scale = max(np.abs(os_[c]).max(), 1e-300)
            assert np.abs(gs[c] - os_[c]).max() <= tol * scale, (step, name, np.abs(gs[c] - os_[c]).max() / scale)
        gc, oc = ge.checksums(), oe.checksums()
        for name, v in oc.items():
            assert abs(gc[name] - v) <= tol * max(abs(v), 1e-300), (step, name, gc[name], v)
        # ions: levels by lattice index (bit-exact integer state)
        greal, gvalid, glev, gkey = ge.ions()
        oreal, ovalid, olev = oe.ions()
        assert sorted(gkey) == list(range(len(olev)))
        assert np.array_equal(glev[np.argsort(gkey)], olev)
        assert np.array_equal(gvalid[np.argsort(gkey)], ovalid)
        # electrons: as many, and the same particles (the device appends them in the order its waves finish)
        n_ion, n_el = ge.ion_stats()
        er, ev = ge.particles()
        orl, ovl = oe.particles()
        assert er.shape == orl.shape and n_el == orl.shape[1] and np.array_equal(np.sort(ev), np.sort(ovl))
        total += int((olev - deck["ion_init_level"]).sum())
        assert n_ion == total == oe.n_ionized()
        if er.shape[1]:
            kg = np.lexsort((np.round(er[1] / deck["hi"][1], 9), np.round(er[0] / deck["hi"][0], 9), np.round(er[2] / er[2].max(), 9)))
            ko = np.lexsort((np.round(orl[1] / deck["hi"][1], 9), np.round(orl[0] / deck["hi"][0], 9), np.round(orl[2] / orl[2].max(), 9)))
            for q in (0, 1, 2, 3, 4, 5):
                sc = max(np.abs(orl[q]).max(), 1e-300)
                assert np.abs(er[q][kg] - orl[q][ko]).max() <= 1e-7 * sc, (step, q)
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("tile_size", [0, 16])
def test_ionization_deck_matches_oracle(api, oracle, tile_size):
    """tests/ionization.2Rank.sh's deck (neutral hydrogen, a flat-top driver, hipace.dt = 1e-12): the oracle is pinned on
    the reference's ionization.2Rank.json to what the random draws leave open (tests/test_oracle_golden.py); the HIP
    engine equals the oracle with the same generator key -- both plasma species, the moving beam, two steps."""
    deck = decks.ionization_SI()
    n = _compare_ion_run(api, oracle, deck, tile_size, 2)
    assert n > 500


@pytest.mark.gpu
@pytest.mark.parametrize("tile_size,solver", [(16, 1), (0, 1), (16, 2)])
def test_laser_wake_with_ionization_matches_oracle(api, oracle, tile_size, solver):
    """BASELINE config 5 at test size: the laser-driven wake in a gas with neutral nitrogen that the wake ionises, the
    envelope advanced by the FFT / multigrid solver over two steps; every slab component, the ion levels and the
    released electrons equal the oracle's."""
    deck = decks.laser_ionization_SI()
    deck.update(nx=64, ny=64, nz=60, laser_solver=solver, dt=6.0 * 10.0e-6 / 299792458.0, n_steps=2)
    n = _compare_ion_run(api, oracle, deck, tile_size, 2, tol=1e-7)
    assert n > 100


@pytest.mark.gpu
def test_ionization_refusals(api):
    deck = decks.ionization_SI()
    with pytest.raises(RuntimeError):
        api.SliceEngine(dict(deck, ion_charge=deck["plasma_charge"]))    # product and ion charges must be opposite
    norm = decks.blowout_wake()
    decks.with_ion_species(norm, "H", 1.0)
    with pytest.raises(RuntimeError):
        api.SliceEngine(norm)                                            # normalised units need background_density_SI


@pytest.mark.gpu
@pytest.mark.parametrize("ts,rho", [(16, 0), (32, 0), (16, 1)])
def test_fused_push_and_deposit_schedule(api, ts, rho):
    """hps_engine_set_fusion: the push of slice k deposits the currents of slice k-1 in the same pass over the sheet.  The
    per-slice checksums (taken when all components of a slice are final) reproduce the reference's fixture exactly as the
    two-kernel schedule does, every slab component that does not belong to the next slice yet equals the two-kernel
    schedule's after each slice, and so does the particle sheet."""
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    deck = decks.blowout_wake()
    deck.update(deposit_rho=rho)
    a = api.SliceEngine(deck, tile_size=ts, sort_period=7)
    b = api.SliceEngine(deck, tile_size=ts, sort_period=7)
    b.set_fusion(True)
    for e in (a, b):
        e.set_diagnostics(True)
        e.begin_step()
    nz = deck["nz"]
    names = a.comp_names()
    ahead = {"jx", "jy", "chi", "rhomjz", "rho", "jx_beam", "jy_beam", "jz_beam", "N_jx_beam", "N_jy_beam", "P_jx_beam", "P_jy_beam"}
    for k in range(nz - 1, -1, -1):
        a.solve_slice(k)
        b.solve_slice(k)
        if k % 9 == 0 or k < 3:
            sa, sb = a.slab(), b.slab()
            for c, nm in enumerate(names):
                if nm in ahead and k > 0:
                    continue
                sc = max(np.abs(sa[c]).max(), 1e-300)
                assert np.abs(sa[c] - sb[c]).max() <= 1e-10 * sc, (k, nm)
            ra, va = a.particles()
            rb, vb = b.particles()
            assert np.array_equal(va, vb)
            for q in range(11):
                assert np.abs(ra[q] - rb[q]).max() <= 1e-10 * max(np.abs(ra[q]).max(), 1e-300), (k, q)
    ca, cb = a.checksums(), b.checksums()
    for nm, v in gold.items():
        if v != 0.0:
            assert abs(cb[nm] - v) <= 1e-9 * abs(v), (nm, cb[nm], v)
    for nm, v in ca.items():
        assert abs(cb[nm] - v) <= 1e-10 * max(abs(v), 1e-300), (nm, cb[nm], v)


@pytest.mark.gpu
def test_openpmd_output_of_the_engine(api, tmp_path):
    """the engine's field diagnostic and beam written in the openPMD hierarchy (hipace_amd/openpmd_writer.py)
    and reduced as the reference's checksum backend does (tests/openpmd_shim.py) reproduce the reference's JSON."""
    import torch
    from hipace_amd import openpmd_writer as W
    from tests import openpmd_shim as S
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))
    deck = decks.blowout_wake()
    eng = api.SliceEngine(deck)
    names = list(gold["lev=0"])
    eng.set_field_diagnostic(names)
    nb, off = eng.beam_layout()
    buf = torch.zeros(7 * nb, dtype=torch.float64, device="cuda")
    eng.initial_beam_into(buf)
    h = buf.cpu().numpy()
    rows = [np.concatenate([h[7 * off[p]:7 * off[p + 1]].reshape(7, -1)[k] for p in range(len(off) - 1)]) for k in range(7)]
    for step in range(deck["n_steps"]):
        eng.run_step()
        W.write_engine_output(eng, str(tmp_path), step, beam=np.stack(rows))
    cs = S.checksums(str(tmp_path))
    for grp in ("lev=0", "beam"):
        for k, v in gold[grp].items():
            assert abs(cs[grp][k] - v) <= 1e-9 * max(abs(v), 1e-300), (grp, k, cs[grp][k], v)
    # the HDF5 files (openpmd_%06T.h5, the reference's container) read by h5py as openPMD-viewer reads them, where the
    # image has an interpreter with h5py (tests/h5py_reader.py)
    hc = S.h5py_checksums(str(tmp_path))
    if hc is not None:
        for grp in ("lev=0", "beam"):
            for k, v in gold[grp].items():
                assert abs(hc[grp][k] - v) <= 1e-9 * max(abs(v), 1e-300), ("h5py", grp, k, hc[grp][k], v)


@pytest.mark.gpu
@pytest.mark.parametrize("tile_size", [0, 16])
def test_plasma_density_profile_matches_oracle(api, oracle, tile_size):
    """InitParticles with a density that depends on (x, y, c t) (PlasmaParticleContainerInit.cpp:246-313), here the
    tabulated form n = n0 f_r(r) f_t(ct): a parabolic plasma channel that ends at r = 6 (no particles beyond) and a
    density up-ramp over three time steps.  Slab and particle sheet equal the oracle's after every step."""
    deck = decks.blowout_wake()
    deck.update(nz=20, lo=(-8.0, -8.0, -1.2), hi=(8.0, 8.0, 1.2), beam_zmin=-1.1, beam_zmax=1.1, n_steps=3, dt=2.0, plasma_ppc=(2, 2),
                beam_umean=(0.0, 0.0, 1.0e6), beam_n_subcycles=1)
    r = np.array([0.0, 1.0, 2.0, 4.0, 6.0, 6.01])
    fr = np.array([1.0, 1.05, 1.2, 1.8, 2.8, 0.0])
    ct, ft = np.array([0.0, 4.0]), np.array([0.25, 1.0])
    ge = api.SliceEngine(deck, tile_size=tile_size)
    oe = oracle.Engine(deck)
    ge.set_density_profile(r, fr, ct, ft)
    oe.set_density_profile(r, fr, ct, ft)
    sums = []
    for step in range(3):
        ge.begin_step()
        oe.begin_step()
        for k in range(deck["nz"] - 1, -1, -1):
            ge.solve_slice(k)
            oe.solve_slice(k)
        gs, os_ = ge.slab(), oe.slab()
        for c, name in enumerate(ge.comp_names()):
            scale = max(np.abs(os_[c]).max(), 1e-300)
            assert np.abs(gs[c] - os_[c]).max() <= 1e-9 * scale, (step, name)
        gr, gv = ge.particles()
        orl, ov = oe.particles()
        keep = gv != 0
        assert keep.sum() == orl.shape[1] == int(ov.sum()) and keep.sum() < gv.size       # the channel's edge removed some
        kg = np.lexsort((np.round(gr[7][keep], 9), np.round(gr[6][keep], 9)))
        ko = np.lexsort((np.round(orl[7], 9), np.round(orl[6], 9)))
        sums.append(orl[2].sum())
        for q in range(11):
            assert np.abs(gr[q][keep][kg] - orl[q][ko]).max() <= 1e-9 * max(np.abs(orl[q]).max(), 1e-300), (step, q)
    assert sums[0] < sums[1] < sums[2] and abs(sums[2] / sums[0] - 4.0) < 0.05         # the ramp: 0.25 -> 0.625 -> 1


@pytest.mark.gpu
def test_beam_spin_tracking_matches_oracle(api, oracle):
    """<beam>.do_spin_tracking: the spin vectors after six steps of a beam that slips through the slices (the partition
    kernel has to carry them along) equal the oracle's, particle by particle."""
    deck = decks.beam_evolution()
    deck.update(nz=12, lo=(-2.0, -2.0, -2.4), hi=(2.0, 2.0, 2.4), beam_zmin=-1.0, beam_zmax=1.6, beam_umean=(0.0, 0.0, 1.2),
                beam_density=1.0e-3, n_steps=6, dt=0.9, beam_n_subcycles=4, ext_E_slope=(0.3, 0.2),
                beam_spin_tracking=1, beam_initial_spin=(1.0, 1.0, 0.5))
    eng = api.SliceEngine(deck, tile_size=0)
    for _ in range(deck["n_steps"]):
        eng.run_step()
    ref = oracle.Engine(deck)
    ref.run()
    bnd, soa = eng.beam_state()
    spin = eng.beam_spin()
    nz = deck["nz"]
    turned = 0.0
    s0 = np.array([1.0, 1.0, 0.5]) / 1.5
    for p in range(nz):
        want, wsp = ref.beam_slice(nz - 1 - p), ref.beam_spin(nz - 1 - p)
        got, gsp = soa[:, bnd[p]:bnd[p + 1]], spin[:, bnd[p]:bnd[p + 1]]
        assert got.shape == want.shape and gsp.shape == wsp.shape
        if want.shape[1]:
            ko = np.lexsort((want[1], want[0])); kg = np.lexsort((got[1], got[0]))
            assert np.abs(got[:, kg] - want[:, ko]).max() <= 1e-10 * np.abs(want).max()
            assert np.abs(gsp[:, kg] - wsp[:, ko]).max() <= 1e-10
            assert np.abs(np.sqrt((gsp ** 2).sum(0)) - 1.0).max() < 1e-12
            turned = max(turned, np.abs(wsp - s0[:, None]).max())
    assert turned > 1e-3            # the deck does make the spins precess
    with pytest.raises(RuntimeError):
        api.SliceEngine(dict(decks.blowout_wake(), beam_spin_tracking=1))       # needs a moving beam


# ---- the multi-rank code path of the ring driver on the one GPU of the box (RcclSelfRing) ------------------------------
@pytest.mark.gpu
def test_ring_driver_on_rccl_static_beam(api):
    """run_pipeline with its hand-off going through RCCL although there is one rank: receives posted a whole step ahead,
    ncclSend behind the engine's event of the slice, the engine's stream waiting for the receive event, blocks reused
    behind their last send -- no host synchronisation per slice.  Three steps (the ring closes twice); every step has the
    reference's checksums, i.e. every block arrived before it was read."""
    import torch
    from hipace_amd.pipeline import RcclSelfRing, run_pipeline
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    deck = decks.blowout_wake()
    eng = api.SliceEngine(deck)
    eng.set_diagnostics(True)
    T = RcclSelfRing(0)
    sums = {}
    solved = run_pipeline(eng, 0, 1, 3, torch.device("cuda", 0), on_step_end=lambda s: sums.__setitem__(s, eng.checksums()), transport=T)
    assert solved == 3 * deck["nz"] and set(sums) == {0, 1, 2}
    st = T.stats()
    nb, off = eng.beam_layout()
    nonempty = int((np.diff(off) > 0).sum())
    assert st["sent"] == st["received"] == 2 * nonempty and st["bytes_sent"] == 2 * 7 * 8 * nb
    for s in (1, 2):
        for k, v in gold.items():
            if v != 0.0:
                assert abs(sums[s][k] - v) <= 1e-9 * abs(v), (s, k, sums[s][k], v)
    T.close()


@pytest.mark.gpu
def test_ring_driver_on_rccl_moving_beam(api, oracle):
    """The same with a beam that slips every step: fixed-size messages packed and unpacked on the device, send slots
    reused behind their send events; per-step checksums equal the oracle stepping the same deck."""
    import torch
    from hipace_amd.pipeline import RcclSelfRing, run_pipeline
    deck = decks.beam_evolution()
    deck.update(nz=12, lo=(-2.0, -2.0, -2.4), hi=(2.0, 2.0, 2.4), beam_zmin=-1.0, beam_zmax=1.6, beam_umean=(0.0, 0.0, 1.2),
                beam_density=1.0e-3, n_steps=4, dt=0.9, beam_n_subcycles=4, ext_E_slope=(0.3, 0.2))
    ref = oracle.Engine(deck)
    want = {}
    for s in range(deck["n_steps"]):
        ref.begin_step()
        for k in range(deck["nz"] - 1, -1, -1):
            ref.solve_slice(k)
        want[s] = ref.checksums()
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_diagnostics(True)
    T = RcclSelfRing(0)
    got = {}
    solved = run_pipeline(eng, 0, 1, deck["n_steps"], torch.device("cuda", 0), on_step_end=lambda s: got.__setitem__(s, eng.checksums()), transport=T)
    assert solved == deck["n_steps"] * deck["nz"] and T.stats()["sent"] == 3 * deck["nz"]
    for s in want:
        for k in ("jz_beam", "jx_beam", "Bx", "By", "Ez", "Sx", "Sy"):
            assert abs(got[s][k] - want[s][k]) <= 1e-9 * max(abs(want[s][k]), 1e-300), (s, k, got[s][k], want[s][k])
    eng.beam_state()
    T.close()


@pytest.mark.gpu
def test_ring_driver_on_rccl_laser(api):
    """... and with an evolving laser pulse: the envelope's two time levels of every slice travel behind the slice's beam
    message (here there is no beam), with a whole step of receive look-ahead; envelope and checksums of four steps equal
    one engine that rotates its own time levels."""
    import torch
    from hipace_amd.pipeline import RcclSelfRing, run_pipeline
    d = decks.laser_blowout_wake()
    d.update(nx=32, ny=32, nz=16, lo=(-16.0, -16.0, -4.0), hi=(16.0, 16.0, 4.0), laser_a0=1.5, laser_lambda0=0.4, laser_solver=1, dt=5.0)
    ref = api.SliceEngine(d)
    ref.set_diagnostics(True)
    want = {}
    for s in range(4):
        ref.run_step()
        want[s] = (ref.checksums(), ref.laser_envelope().copy())
    eng = api.SliceEngine(d)
    eng.set_diagnostics(True)
    T = RcclSelfRing(0)
    got = {}
    run_pipeline(eng, 0, 1, 4, torch.device("cuda", 0), on_step_end=lambda s: got.__setitem__(s, (eng.checksums(), eng.laser_envelope().copy())), transport=T)
    assert T.stats()["sent"] == 2 * 3 * d["nz"]        # per slice: the (empty) moving-beam message and the envelope
    for s in range(4):
        assert np.abs(got[s][1] - want[s][1]).max() <= 1e-12 * np.abs(want[s][1]).max(), s
        for k, v in want[s][0].items():
            assert abs(got[s][0][k] - v) <= 1e-10 * max(abs(v), 1e-300), (s, k)
    T.close()


def _run_with_env(api, var, value, deck, n_steps, tile_size=16):
    """one engine created with an HPS_* switch set (the library reads them when the engine is created)"""
    old = os.environ.get(var)
    os.environ[var] = value
    try:
        e = api.SliceEngine(deck, tile_size=tile_size, sort_period=7)
    finally:
        if old is None:
            del os.environ[var]
        else:
            os.environ[var] = old
    for _ in range(n_steps):
        e.begin_step()
        for k in range(deck["nz"] - 1, -1, -1):
            e.solve_slice(k)
    e.sync()
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gated_push", "lazy_shift", "fuse_sources", "aux_stream", "fold_beam", "fold_hierarchy", "laser_stream_fft", "laser_stream_mg", "ion_tile_skip", "fold_tail", "gated_ion_push", "poisson_tridiag", "poisson_tridiag_dense", "poisson_tridiag_pow2", "pc_speculate", "valid_by_w", "valid_by_psi", "cu_masks", "post_in_push"])
def test_schedules_do_not_change_results(api, case):
    """The engine's scheduling choices -- the push enqueued behind the multigrid's V-cycles and gated on its stopping rule,
    the envelope solver on a stream of its own, the tiles of atoms that cannot ionise skipped before their image is loaded --
    against the plain schedule (each has an HPS_* switch): same slab, same particles, same envelope, same ion levels and
    released electrons.  No diagnostics here: they would keep the gated push off."""
    if case == "gated_push":
        var, deck, steps = "HPS_GATED_PUSH", decks.blowout_wake(), 1
    elif case == "lazy_shift":      # ShiftSlices deferred into the next slice's InitializeSlices pass
        var, deck, steps = "HPS_LAZY_SHIFT", decks.blowout_wake(), 1
    elif case == "fuse_sources":    # the Poisson sources formed inside the first transform pass (no k_rhs_all, no staging planes)
        var, deck, steps = "HPS_FUSE_SOURCES", decks.blowout_wake(), 1
    elif case == "fold_beam":       # the static beam's deposits as extra workgroups of the plasma's deposition
        var, deck, steps = "HPS_FOLD_BEAM", decks.blowout_wake(), 2
    elif case == "fold_hierarchy":  # the multigrid's coefficient hierarchy in the launch of the -grad Psi / Sx, Sy pass
        var, deck, steps = "HPS_FOLD_HIERARCHY", decks.blowout_wake(), 2
    elif case == "aux_stream":      # the beam's deposition and the multigrid's coefficient hierarchy on a stream beside the slice's
        var, deck, steps = "HPS_AUX_STREAM", decks.blowout_wake(), 2
    elif case == "valid_by_w":       # the depositions read "weight != 0" instead of the valid bit of idcpu
        var, deck, steps = "HPS_VALID_BY_W", decks.blowout_wake(), 2
    elif case == "valid_by_psi":     # the push reads "psi_half != 0" instead of the valid bit of idcpu (absorbing walls: particles do die)
        var, deck, steps = "HPS_VALID_BY_PSI", dict(decks.blowout_wake(), bc=2), 2
    elif case.startswith("poisson_tridiag"):
        # round 6: the y direction of every Poisson solve as tridiagonal solves (k_tridiag_y) against the rocFFT back-end's forward
        # DST, inverse eigenvalues, inverse DST -- the same discrete operator -- behind the own transform (65 = 5 x 13), the dense
        # products (61 cells: 62 has no built factorisation) and the power-of-two kernel (63 cells).  (With rocFFT the sources
        # come through k_rhs_all and staging planes: that solver cannot form them itself.)
        var, steps = "HPS_POISSON_BACKEND", 1
        deck = decks.blowout_wake()
        if case.endswith("dense"):
            deck.update(nx=61, ny=61)
        elif case.endswith("pow2"):
            deck.update(nx=63, ny=63)
    elif case == "pc_speculate":     # predictor-corrector loop: iterations enqueued ahead, every kernel gated on the loop's condition
        var, steps = "HPS_PC_SPECULATE", 1
        deck = decks.predictor_corrector(decks.linear_wake_gaussian(), 4.0e-2, 30, 0.05)
        deck.update(nx=64, ny=64, nz=60, plasma_ppc=(2, 2), beam_zmin=deck["lo"][2], beam_zmax=deck["hi"][2])      # (beam on every slice: no loop on rounding noise)
    elif case.startswith("laser_stream"):
        var, steps = "HPS_LASER_ASYNC", 3
        deck = decks.laser_blowout_wake()
        deck.update(nx=64, ny=64, nz=30, lo=(-16.0, -16.0, -4.0), hi=(16.0, 16.0, 4.0), laser_a0=1.5, laser_lambda0=0.4,
                    laser_solver=1 if case.endswith("fft") else 2, dt=5.0, n_steps=3)
    elif case == "post_in_push":    # the gated push posts the Bx/By solve's norms to the host itself (no k_post_norms launch ahead of it)
        var, deck, steps = "HPS_POST_IN_PUSH", decks.blowout_wake(), 2
    elif case == "cu_masks":        # (diagnostic: the engine's stream on half of the compute units, hipExtStreamCreateWithCUMask; "0": a plain stream)
        var, deck, steps = "HPS_CU_MASKS", decks.blowout_wake(), 1
    else:      # fold_tail: the electrons released since the last sort ride in the tile kernels' launches (sort_period 7: tails of up to 6 slices)
        # gated_ion_push: the ions' push (with its ADK decisions) and the electrons' push enqueued behind the Bx/By V-cycles
        var, steps = {"ion_tile_skip": "HPS_ION_TILE_SKIP", "fold_tail": "HPS_FOLD_TAIL", "gated_ion_push": "HPS_GATED_ION_PUSH"}[case], 2
        deck = decks.laser_ionization_SI()
        deck.update(nx=128, ny=128, nz=60, laser_solver=1, dt=6.0 * 10.0e-6 / 299792458.0, n_steps=2)
    on, off = ("rocfft", "own") if case.startswith("poisson_tridiag") else ("0-127" if case == "cu_masks" else "1", "0")
    a = _run_with_env(api, var, on, deck, steps)
    b = _run_with_env(api, var, off, deck, steps)
    sa, sb = a.slab(), b.slab()
    # two runs of ONE schedule differ by the order of their LDS atomics; two steps of the ionisation deck have shown 1.2e-12
    # (the predictor-corrector loop amplifies that order through its ~5 dependent solves per slice: Bz, five orders of magnitude
    #  below the other fields in this deck, has shown 4e-12)
    # (the two forms of the y solve are the same operator with other rounding: 1e-13 per solve, carried by the particles down the box)
    tol = 1e-11 if case in ("ion_tile_skip", "fold_tail", "gated_ion_push") else 1e-10 if (case == "pc_speculate" or case.startswith("poisson_tridiag")) else 1e-12
    for c, nm in enumerate(a.comp_names()):
        sc = max(np.abs(sb[c]).max(), 1e-300)
        assert np.abs(sa[c] - sb[c]).max() <= tol * sc, (case, nm)
    ra, va = a.particles()
    rb, vb = b.particles()
    assert ra.shape == rb.shape and np.array_equal(np.sort(va), np.sort(vb))
    if case in ("ion_tile_skip", "fold_tail", "gated_ion_push"):      # (released electrons are appended in the order of an atomic counter)
        (_, _, la, ka), (_, _, lb, kb) = a.ions(), b.ions()
        assert np.array_equal(la[np.argsort(ka)], lb[np.argsort(kb)])
        assert a.ion_stats() == b.ion_stats() and a.ion_stats()[0] > 100
    else:
        assert np.abs(ra - rb).max() <= (1e-10 if (case == "pc_speculate" or case.startswith("poisson_tridiag")) else 1e-12) * np.abs(rb).max()
    if case == "pc_speculate":
        assert a.pc_stats()[0] == b.pc_stats()[0] > deck["nz"]         # the same number of loop iterations, more than one per slice
    if case.startswith("laser_stream"):
        ea, eb = a.laser_envelope(), b.laser_envelope()
        assert np.abs(ea - eb).max() <= 1e-13 * np.abs(eb).max()
        assert a.laser_vcycles() == b.laser_vcycles()


@pytest.mark.gpu
@pytest.mark.parametrize("tile_size", [0, 16])
def test_mobile_ions_match_oracle(api, oracle, tile_size):
    """examples/linear_wake/inputs_ion_motion_SI (tests/ion_motion.SI.1Rank.sh) with a deterministic driver: electrons and
    mobile ions of 5 electron masses, one particle per cell each, neither with a neutralising background -- the second
    species at its top level (nothing to ionise).  Every slab component, both sheets and the ions' levels equal the
    oracle's; the ions do move."""
    deck = decks.ion_motion_SI(60)
    n = _compare_ion_run(api, oracle, deck, tile_size, 1)
    assert n == 0
    ge = api.SliceEngine(deck, tile_size=tile_size)
    ge.begin_step()
    for k in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(k)
    real, valid, lev, _ = ge.ions()
    assert lev.min() == 1 and lev.max() == 1
    assert np.abs(real[3]).max() > 1e6          # transverse momentum of the ions (u = gamma v, SI)


@pytest.mark.gpu
@pytest.mark.parametrize("edge", ["rccl", "ipc"])
def test_cpp_host_runs_the_ring_through_the_c_abi(api, tmp_path, edge):
    """examples/ring_host.cpp: a C++ program above include/hpslice.h (no Python, no torch in the process) that runs three
    time steps of the blowout_wake deck slice by slice and hands every beam block of a step to the next one through the
    ring (HPS_RING_EDGE: RCCL's ncclSend + ncclRecv, or the ipc edge's copy on the ring's stream), ordered by events -- the loop
    a maintainer of the reference would write in Hipace::Evolve.  Every step reproduces the reference's checksums, and 2/3 of
    all beam bytes went through the ring."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "ring_host")
    if not os.path.exists(exe):                          # normally built by __graft_entry__.build()
        import __graft_entry__
        __graft_entry__.build_cpp_host()
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    deck = decks.blowout_wake()
    eng = api.SliceEngine(deck)
    names = eng.comp_names()
    nbeam, _ = eng.beam_layout()
    path = tmp_path / "deck.bin"
    path.write_bytes(bytes(eng._dk))                     # the hps_deck the engine was created from
    del eng
    out = subprocess.run([exe, str(path), "3", "16"], capture_output=True, text=True, timeout=600, env=dict(os.environ, HPS_RING_EDGE=edge))
    assert out.returncode == 0, out.stderr[-2000:]
    steps = [l.split() for l in out.stdout.splitlines() if l.startswith("step ")]
    assert [int(s[1]) for s in steps] == [0, 1, 2]
    for s in steps:
        cs = dict(zip(names, map(float, s[2:])))
        for k, v in gold.items():
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (s[1], k, cs[k], v)
    ring = [l.split() for l in out.stdout.splitlines() if l.startswith("ring ")][0]
    assert int(ring[1]) == int(ring[2]) > 0 and int(ring[3]) == 2 * 7 * 8 * nbeam


@pytest.mark.gpu
@pytest.mark.parametrize("stages,n_steps", [(1, 2), (2, 3), (3, 7)])
def test_cpp_pipeline_host_with_several_stages_per_rank(api, tmp_path, stages, n_steps):
    """examples/pipeline_host.cpp: the multi-rank C++ host (rank / world / edge ids through files; several stages per rank
    on in-process edges, the RCCL ring between processes, one host thread, slices in two halves) run as one rank: every
    step -- open and closed ring -- reproduces the reference's checksums.  (Two ranks need two GPUs: RCCL refuses two ranks on
    one device; the between-process branch of this host has not run.)"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pipeline_host")
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build_cpp_host()
    gold = json.load(open(os.path.join(GOLD, "blowout_wake_explicit.2Rank.json")))["lev=0"]
    eng = api.SliceEngine(decks.blowout_wake())
    names = eng.comp_names()
    path = tmp_path / "deck.bin"
    path.write_bytes(bytes(eng._dk))
    del eng
    out = subprocess.run([exe, str(path), str(n_steps), "0", "1", str(tmp_path), str(stages)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    steps = [l.split() for l in out.stdout.splitlines() if l.startswith("step ")]
    assert sorted(int(s[1]) for s in steps) == list(range(n_steps))
    for s in steps:
        cs = dict(zip(names, map(float, s[2:])))
        for k, v in gold.items():
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (s[1], k, cs[k], v)
