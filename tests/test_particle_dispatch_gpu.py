"""Every kernel instance the four tiled particle dispatchers of particles_tiled.hip can launch without environment switches,
against the oracle and, for the deposition, the float64 numpy reference of tests/util.py.

The dispatchers choose by order (0..3) x tile size (16, 32) and then
  * deposit_current_tiled:  a laser (mask 51 or any other set), the valid-by-weight ("VBW") variants of masks 51 and 3, else
                            one instance per mask 51, 59, 32, 3, 39, 47 and the generic one (-1);
  * explicit_deposit_tiled: derivative_type 1 / 2 x laser, and the VBW variant of derivative_type 2 without a laser;
  * advance_plasma_tiled:   laser x ionisation (ADK, the engine's ion species only) x valid-by-psi_half ("VBP": order 2 on
                            16 x 16 tiles only);
  * advance_deposit_tiled:  the fused push + deposition of masks 51 / 59 (k_advance_tiled<2, 16, .., DEP> for order 2 on
                            16 x 16 tiles, k_advance_deposit_tiled otherwise), reached through SliceEngine.set_fusion.
Every case states the instance it must launch (hps_particles_record), and test_every_kernel_of_the_dispatch_is_reached
holds the record of a pass over all of them to the list below, so a change of the dispatch fails here instead of leaving a
kernel without a test.

Not reached here (environment switches only): HPS_EXPL_PAD=8 (k_explicit_tiled<.., 8, 0>), HPS_FUSED_KERNEL=old at order 2 on
16 x 16 tiles and HPS_FUSED_THREADS=512 (k_advance_deposit_tiled<.., 512>), HPS_CELL_BLOCK_W (the sort's cell numbering).

The sheets hold particles exactly on tile borders and on the domain walls, invalid particles (w = 0, psi_half = 0: the
promise Tiling.set_validity states), and QSA violators (psi < 0, psi = 0, gamma/psi > 35) both near their home tile (LDS
path) and moved away from it after the sort (the slab path of a stale sort).  The grids are not multiples of the tile size,
give non-square tile grids, or are smaller than one tile."""
import numpy as np
import pytest

from hipace_amd import decks
from tests.util import DEP_COMPS, NCOMP, deposit_current_ref, deposit_weights, rel_err, smooth_slab, thermal_sheet

pytestmark = pytest.mark.gpu

LO, HI = (-8.0, -8.0), (8.0, 8.0)
DEP = [15, 16, 3, 18, 2, 17]                 # jx jy jz rho chi rhomjz
CACHE, SRC = [10, 7, 5, 6], [3, 4]           # Bz Ez ExmBy EypBx -> Sy Sx
PUSH = [11, 7, 8, 9, 10]                     # Psi Ez Bx By Bz
AABS = 20
ORDERS, TILES = (0, 1, 2, 3), (16, 32)
GRIDS = [(100, 72), (127, 65), (17, 9), (1023, 64)]
MASKS = (51, 59, 32, 3, 39, 47, 28)          # 28 (jz rho chi): the generic instance


def _b(v):
    return int(bool(v))


def dep_name(o, s, mask, laser, vbw):
    m = mask if (mask in (51, 59, 32, 3, 39, 47) and not laser) or (laser and mask == 51) else -1
    return f"k_deposit_tiled<{o},{s},{m},{_b(laser)},{_b(vbw)}>"


def expl_name(o, dt, s, laser, vbw):
    return f"k_explicit_tiled<{o},{dt},{s},{_b(laser)},2,{_b(vbw)}>"


def push_name(o, s, laser, ionize, vbp, dep=0):
    return f"k_advance_tiled<{o},{s},{_b(laser)},{_b(ionize)},{_b(vbp)},{dep}>"


def fused_name(o, s, rho):
    mask = 59 if rho else 51
    return push_name(2, 16, 0, 0, 0, mask) if (o, s) == (2, 16) else f"k_advance_deposit_tiled<{o},{s},{mask},256>"


# every instance reachable without environment switches
EXPECTED = sorted(
    [dep_name(o, s, m, 0, 0) for o in ORDERS for s in TILES for m in MASKS]
    + [dep_name(o, s, m, 1, 0) for o in ORDERS for s in TILES for m in (51, 28)]
    + [dep_name(o, s, m, 0, 1) for o in ORDERS for s in TILES for m in (51, 3)]
    + [expl_name(o, dt, s, la, 0) for o in ORDERS for s in TILES for dt in (1, 2) for la in (0, 1)]
    + [expl_name(o, 2, s, 0, 1) for o in ORDERS for s in TILES]
    + [push_name(o, s, la, io, 0) for o in ORDERS for s in TILES for la in (0, 1) for io in (0, 1)]
    + [push_name(2, 16, la, 0, 1) for la in (0, 1)]
    + [fused_name(o, s, r) for o in ORDERS for s in TILES for r in (0, 1)])

# ---- case tables: (order, tile, variant..., grid, stale sort, can_ionize) --------------------------------------------------
DEP_CASES = []
for _o in ORDERS:
    for _s in TILES:
        for _m, _la, _v in [(m, 0, 0) for m in MASKS] + [(51, 1, 0), (28, 1, 0), (51, 0, 1), (3, 0, 1)]:
            _k = len(DEP_CASES)
            DEP_CASES.append((_o, _s, _m, _la, _v, GRIDS[_k % 4], (_k // 4) % 2 == 0, _k % 3 != 1))
EXPL_CASES = []
for _o in ORDERS:
    for _s in TILES:
        for _dt, _la, _v in [(1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 1, 0), (2, 0, 1)]:
            _k = len(EXPL_CASES)
            EXPL_CASES.append((_o, _s, _dt, _la, _v, GRIDS[_k % 4], (_k // 4) % 2 == 0, _k % 3 != 1))
PUSH_CASES = []
for _o in ORDERS:
    for _s in TILES:
        for _la in (0, 1):
            for _v in ((0, 1) if (_o, _s) == (2, 16) else (0,)):
                for _r in range(2):
                    _k = len(PUSH_CASES)
                    # (bc, n_subcycles, temp_slice) rotate through 0/1/2 x 1/2/3 x 0/1
                    PUSH_CASES.append((_o, _s, _la, _v, (_k % 3, 1 + (_k // 3) % 3, (_k // 2) % 2), GRIDS[_k % 4],
                                       (_k // 4) % 2 == 0, (_k % 3 != 1) and not _v))


def _dep_id(c):
    o, s, m, la, v, (nx, ny), stale, io = c
    return f"o{o}-t{s}-m{m}" + ("-laser" if la else "") + ("-vbw" if v else "") + f"-{nx}x{ny}" + ("-stale" if stale else "") + \
        ("-ion" if io else "")


def _expl_id(c):
    o, s, dt, la, v, (nx, ny), stale, io = c
    return f"o{o}-t{s}-dt{dt}" + ("-laser" if la else "") + ("-vbw" if v else "") + f"-{nx}x{ny}" + ("-stale" if stale else "") + \
        ("-ion" if io else "")


def _push_id(c):
    o, s, la, v, (bc, nsub, temp), (nx, ny), stale, io = c
    return f"o{o}-t{s}" + ("-laser" if la else "") + ("-vbp" if v else "") + f"-bc{bc}-sub{nsub}-temp{temp}-{nx}x{ny}" + \
        ("-stale" if stale else "") + ("-ion" if io else "")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    yield A
    A.record_particle_dispatch(False)


class Setup:
    """A tile-sorted sheet on an nx x ny grid with its tiling, a slab of smooth fields, the oracle's geometry."""

    def __init__(self, api, oracle, nx, ny, ts, order, seed, stale, ionize, violators, bc=1, dz=0.3):
        rng = np.random.default_rng(seed)
        self.nx, self.ny, self.g = nx, ny, (order + 1) // 2 + 1
        self.geom = api.Geometry(nx, ny, LO, HI, dz, bc=bc)
        self.ogeom = oracle.make_geom(nx, ny, LO, HI, dz=dz, bc=bc)
        real, valid, ion = thermal_sheet(nx, ny, LO, HI, ppc=1 if nx * ny > 20000 else 2, seed=seed, u_std=0.3)
        n = real.shape[1]
        dx, dy = (HI[0] - LO[0]) / nx, (HI[1] - LO[1]) / ny
        # exactly on tile borders (the face between the last cell of a tile and the first of the next, and the centre of
        # a tile's first cell), on the walls lo and hi, and in the corners
        bx = [LO[0] + ts * m * dx for m in range(1, (nx - 1) // ts + 1)] + [LO[0] + (ts * m + 0.5) * dx for m in range(0, nx // ts)]
        by = [LO[1] + ts * m * dy for m in range(1, (ny - 1) // ts + 1)] + [LO[1] + (ts * m + 0.5) * dy for m in range(0, ny // ts)]
        edge = rng.choice(n, 64, replace=False)
        xs = np.array(bx + [LO[0], HI[0]])
        ys = np.array(by + [LO[1], HI[1]])
        real[0, edge] = xs[np.arange(64) % xs.size]
        real[1, edge] = ys[(np.arange(64) // 2) % ys.size]
        if order == 0:
            # the order-0 shape jumps at a cell face, where one rounding of (x - xoff)/dx (an FMA on the GPU) picks the
            # cell: there the particles sit 1e-9 cells to either side of the face, inside the walls
            side = np.where(np.arange(64) % 4 < 2, 1.0, -1.0)
            real[0, edge] = np.clip(real[0, edge] + side * 1e-9 * dx, LO[0] + 1e-9 * dx, HI[0] - 1e-9 * dx)
            real[1, edge] = np.clip(real[1, edge] - side * 1e-9 * dy, LO[1] + 1e-9 * dy, HI[1] - 1e-9 * dy)
        real[6], real[7] = real[0], real[1]
        til = api.Tiling(nx, ny, ts, n)
        sheet = til.reorder(api.PlasmaSheet(real, valid, ion), self.geom)
        r, v = sheet.numpy()
        if stale:   # every 5th particle far from its home tile, without re-sorting: the kernels' slab path
            idx = np.arange(0, n, 5)
            r[0, idx] = rng.uniform(LO[0], HI[0], idx.size)
            r[1, idx] = rng.uniform(LO[1], HI[1], idx.size)
            r[6], r[7] = r[0], r[1]
        bad = rng.random(n) < 0.04                   # invalid particles: w = 0 and psi_half = 0 (Tiling.set_validity)
        v[bad] = 0
        r[2, bad] = 0.0
        r[10, bad] = 0.0
        self.nviol = 0
        if violators:   # QSA violators among the particles kept near their tile and among the moved ones
            cand = np.nonzero(~bad)[0]
            near = cand[cand % 5 != 0][:15] if stale else cand[:15]
            far = cand[cand % 5 == 0][:15] if stale else cand[15:30]
            for grp in (near, far):
                r[5, grp[:5]] = -0.3                 # psi < 0
                r[5, grp[5:10]] = 0.0                # psi = 0, ux and uy != 0: gamma/psi = inf
                r[3, grp[5:10]], r[4, grp[5:10]] = 0.2, -0.1
                r[5, grp[10:15]] = 0.05              # gamma/psi > 35 (unless the level is 0)
        self.ion = rng.integers(0, 6, n).astype(np.int32) if ionize else np.zeros(n, dtype=np.int32)
        self.ionize = ionize
        self.real, self.valid, self.til = r, v.astype(np.int32), til
        self.slab = smooth_slab(nx, ny, self.g, amp=0.2)
        self.slab[AABS] = 3.0 * np.abs(self.slab[AABS])      # |a|^2 >= 0

    def sheet(self, api):
        return api.PlasmaSheet(self.real, self.valid, self.ion)


def _check_invariant(pl):
    """Every particle whose valid bit is clear has w == 0 and psi_half == 0 (what the VBW / VBP variants rely on)."""
    r, v = pl.numpy()
    dead = v == 0
    assert np.all(r[2][dead] == 0.0), "an invalid particle kept its weight"
    assert np.all(r[10][dead] == 0.0), "an invalid particle kept its psi_half"
    return int(dead.sum())


def _check_fallback(S, ts, stale):
    """A fresh sort keeps every particle in its tile's image; a stale one sends some through the slab path -- unless one
    tile's image (tile + 2 x 6 halo cells) covers the whole grid."""
    if not stale:
        assert S.til.fallback.item() == 0
    elif max(S.nx, S.ny) > ts + 12:
        assert S.til.fallback.item() > 0


def _run_recorded(api, fn):
    import torch
    api.record_particle_dispatch(True)
    try:
        fn()
        torch.cuda.synchronize()
        return api.recorded_particle_dispatch()
    finally:
        api.record_particle_dispatch(False)


def _deposit(api, S, order, mask, laser, vbw, slab, cnt):
    from hipace_amd import api as A
    comp = [c if (mask >> k) & 1 else -1 for k, c in enumerate(DEP)]
    S.til.set_validity(by_weight=vbw)
    pl, f = S.sheet(api), api.Fields(S.nx, S.ny, S.g, NCOMP, data=slab)
    S.til.fallback.zero_()
    rec = _run_recorded(api, lambda: A.DepositCurrent(pl, f, S.geom, -1.0, 1.0, order, *comp, n_qsa=cnt, can_ionize=S.ionize,
                                                      tiling=S.til, aabs=AABS if laser else -1))
    return comp, pl, f, rec


@pytest.mark.parametrize("case", DEP_CASES, ids=_dep_id)
def test_deposit_tiled(api, oracle, case):
    import torch
    order, ts, mask, laser, vbw, (nx, ny), stale, ionize = case
    S = Setup(api, oracle, nx, ny, ts, order, 100 + nx + order * 7 + mask, stale, ionize, violators=True)
    slab = S.slab.copy()
    slab[DEP] = 0.0
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    comp, pl, f, rec = _deposit(api, S, order, mask, laser, vbw, slab, cnt)
    assert rec == {dep_name(order, ts, mask, laser, vbw)}
    out = f.numpy()
    aabs = AABS if laser else -1
    o, r2, v2 = slab.copy(), S.real.copy(), S.valid.copy()
    nq = oracle.deposit_current(o, nx, ny, S.g, r2, v2, S.ion, S.ogeom, comp, -1.0, 1.0, order, can_ionize=ionize, aabs=aabs)
    ref, rv, rw, rq = deposit_current_ref(slab, S.g, S.real, S.valid, S.ion, S.ogeom, comp, -1.0, 1.0, order, can_ionize=ionize, aabs=aabs)
    live, _, wc, rho, _ = deposit_weights(S.real, S.valid, S.ion, slab, S.g, S.ogeom, -1.0, 1.0, order, can_ionize=ionize, aabs=aabs)
    for k, c in enumerate(comp):
        if c < 0:
            continue
        assert np.abs(o[c]).max() > 0.0
        assert rel_err(out[c], o[c]) < 1e-12, (DEP_COMPS[k], rel_err(out[c], o[c]))
        assert rel_err(out[c], ref[c]) < 1e-12, (DEP_COMPS[k], rel_err(out[c], ref[c]))
        # the shape factors sum to one: slab + guards hold exactly the surviving particles' charge x weight
        terms = rho[live] * wc[k][live]
        assert abs(out[c].sum() - terms.sum()) <= 1e-12 * np.abs(terms).sum(), DEP_COMPS[k]
    rest = [c for c in range(NCOMP) if c not in comp]
    assert np.array_equal(out[rest], slab[rest]), "a component that is not deposited was written"
    assert int(cnt.item()) == nq == rq and rq >= 30
    greal, gvalid = pl.numpy()
    assert np.array_equal(gvalid, v2) and np.array_equal(gvalid, rv)
    assert np.array_equal(greal[2], rw)
    _check_invariant(pl)
    _check_fallback(S, ts, stale)


@pytest.mark.parametrize("case", EXPL_CASES, ids=_expl_id)
def test_explicit_deposit_tiled(api, oracle, case):
    from hipace_amd import api as A
    order, ts, dt, laser, vbw, (nx, ny), stale, ionize = case
    S = Setup(api, oracle, nx, ny, ts, order, 300 + nx + order * 7 + dt, stale, ionize, violators=False)
    S.til.set_validity(by_weight=vbw)
    pl, f = S.sheet(api), api.Fields(nx, ny, S.g, NCOMP, data=S.slab)
    aabs = AABS if laser else -1
    S.til.fallback.zero_()
    rec = _run_recorded(api, lambda: A.ExplicitDeposition(pl, f, S.geom, -1.0, 1.0, order, *CACHE, *SRC, derivative_type=dt,
                                                          can_ionize=ionize, tiling=S.til, aabs=aabs))
    assert rec == {expl_name(order, dt, ts, laser, vbw)}
    out = f.numpy()
    o = S.slab.copy()
    oracle.explicit_deposit(o, nx, ny, S.g, S.real.copy(), S.valid.copy(), S.ion, S.ogeom, CACHE, SRC, -1.0, 1.0, order, dt,
                            can_ionize=ionize, aabs=aabs)
    for c in SRC:
        assert rel_err(out[c] - S.slab[c], o[c] - S.slab[c]) < 1e-12, (c, rel_err(out[c] - S.slab[c], o[c] - S.slab[c]))
    rest = [c for c in range(NCOMP) if c not in SRC]
    assert np.array_equal(out[rest], S.slab[rest]), "a component that is not a source was written"
    _check_fallback(S, ts, stale)


@pytest.mark.parametrize("case", PUSH_CASES, ids=_push_id)
def test_push_tiled(api, oracle, case):
    from hipace_amd import api as A
    order, ts, laser, vbp, (bc, nsub, temp), (nx, ny), stale, ionize = case
    S = Setup(api, oracle, nx, ny, ts, order, 500 + nx + order * 7 + bc, stale, ionize, violators=False, bc=bc)
    S.til.set_validity(by_psi_half=vbp)
    pl, f = S.sheet(api), api.Fields(nx, ny, S.g, NCOMP, data=S.slab)
    aabs = AABS if laser else -1
    rec = _run_recorded(api, lambda: A.AdvancePlasmaParticles(pl, f, S.geom, -1.0, 1.0, order, *PUSH, temp_slice=temp,
                                                              n_subcycles=nsub, can_ionize=ionize, tiling=S.til, aabs=aabs))
    assert rec == {push_name(order, ts, laser, 0, vbp)}
    r2, v2 = S.real.copy(), S.valid.copy()
    oracle.advance_plasma(S.slab, nx, ny, S.g, r2, v2, S.ion, S.ogeom, PUSH, -1.0, 1.0, order, temp, nsub, can_ionize=ionize,
                          aabs=aabs)
    greal, gvalid = pl.numpy()
    assert np.array_equal(gvalid, v2)
    live = v2 != 0
    for k in range(11):
        assert rel_err(greal[k][live], r2[k][live]) < 1e-10, (k, rel_err(greal[k][live], r2[k][live]))
    assert np.array_equal(f.numpy(), S.slab)
    dead = _check_invariant(pl)
    if bc == 2:
        assert dead > int((S.valid == 0).sum()), "no particle was absorbed"


@pytest.mark.parametrize("path", ["deposit-tiled", "deposit-tiled-vbw", "deposit-untiled", "push-tiled", "push-tiled-vbp",
                                  "push-untiled"])
@pytest.mark.parametrize("stale", [False, True])
def test_invalid_particles_have_no_weight_and_no_psi_half(api, oracle, path, stale):
    """Each path that can clear a valid bit -- the QSA drop of the depositions (LDS and slab path), the absorbing boundary of
    the pushes -- also zeroes w and psi_half: the engine's valid-by-weight / valid-by-psi_half variants rely on it."""
    import torch
    from hipace_amd import api as A
    S = Setup(api, oracle, 100, 72, 16, 2, 77, stale, False, violators=path.startswith("deposit"), bc=2, dz=0.6)
    before = int((S.valid == 0).sum())
    pl, f = S.sheet(api), api.Fields(100, 72, S.g, NCOMP, data=S.slab)
    tiled = "untiled" not in path
    S.til.set_validity(by_weight=path.endswith("vbw"), by_psi_half=path.endswith("vbp"))
    S.til.fallback.zero_()
    if path.startswith("deposit"):
        A.DepositCurrent(pl, f, S.geom, -1.0, 1.0, 2, *DEP, tiling=S.til if tiled else None)
    else:
        A.AdvancePlasmaParticles(pl, f, S.geom, -1.0, 1.0, 2, *PUSH, tiling=S.til if tiled else None)
    torch.cuda.synchronize()
    assert _check_invariant(pl) > before
    if tiled:
        _check_fallback(S, 16, stale)


def _small_blowout(order, rho, nz=30):
    deck = decks.blowout_wake()
    deck.update(order=order, deposit_rho=rho, nz=nz, n_steps=1, lo=(-8.0, -8.0, -1.8), hi=(8.0, 8.0, 1.8), beam_zmin=-1.7,
                beam_zmax=2.5)
    return deck


@pytest.mark.parametrize("rho", [0, 1])
@pytest.mark.parametrize("ts", TILES)
@pytest.mark.parametrize("order", ORDERS)
def test_fused_push_and_deposit(api, oracle, order, ts, rho):
    """SliceEngine.set_fusion: the fused push + deposition against the two-kernel schedule after every slice (as
    test_fused_push_and_deposit_schedule does for the deck's order 2), and against the oracle's engine at orders 1 and 3."""
    deck = _small_blowout(order, rho)
    a = api.SliceEngine(deck, tile_size=ts, sort_period=7)
    b = api.SliceEngine(deck, tile_size=ts, sort_period=7)
    b.set_fusion(True)
    for e in (a, b):
        e.begin_step()
    names = a.comp_names()
    ahead = {"jx", "jy", "chi", "rhomjz", "rho", "jx_beam", "jy_beam", "jz_beam", "N_jx_beam", "N_jy_beam", "P_jx_beam", "P_jy_beam"}
    api.record_particle_dispatch(True)
    try:
        for k in range(deck["nz"] - 1, -1, -1):
            a.solve_slice(k)
            b.solve_slice(k)
            if k % 7 == 0:
                sa, sb = a.slab(), b.slab()
                for c, nm in enumerate(names):
                    if nm in ahead and k > 0:
                        continue
                    assert np.abs(sa[c] - sb[c]).max() <= 1e-10 * max(np.abs(sa[c]).max(), 1e-300), (k, nm)
                ra, va = a.particles()
                rb, vb = b.particles()
                assert np.array_equal(va, vb)
                for q in range(11):
                    assert np.abs(ra[q] - rb[q]).max() <= 1e-10 * max(np.abs(ra[q]).max(), 1e-300), (k, q)
        b.sync()
        assert fused_name(order, ts, rho) in api.recorded_particle_dispatch()
    finally:
        api.record_particle_dispatch(False)
    rb, vb = b.particles()
    assert np.all(rb[2][vb == 0] == 0.0) and np.all(rb[10][vb == 0] == 0.0)
    if order in (1, 3):
        oe = oracle.Engine(deck)
        oe.begin_step()
        for k in range(deck["nz"] - 1, -1, -1):
            oe.solve_slice(k)
        gs, os_ = b.slab(), oe.slab()
        for c in range(b.ncomp):
            assert rel_err(gs[c], os_[c]) < 1e-9, (names[c], rel_err(gs[c], os_[c]))


def _engine_slices(api, deck, ts, nslices, fusion=False):
    e = api.SliceEngine(deck, tile_size=ts, sort_period=7)
    if fusion:
        e.set_fusion(True)
    e.begin_step()
    for k in range(deck["nz"] - 1, deck["nz"] - 1 - nslices, -1):
        e.solve_slice(k)
    e.sync()


def test_every_kernel_of_the_dispatch_is_reached(api, oracle):
    """One pass over every case table on small sheets, the fused schedule, and the ionisable species of
    test_ionization_deck_matches_oracle's deck (the push with ADK ionisation exists in the engine only), with and without a
    laser: the instances launched equal EXPECTED."""
    import torch
    from hipace_amd import api as A
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    api.record_particle_dispatch(True)
    try:
        for order, ts, mask, laser, vbw, _, stale, ionize in DEP_CASES:
            S = Setup(api, oracle, 40, 24, ts, order, 1, stale, ionize, violators=True)
            comp = [c if (mask >> k) & 1 else -1 for k, c in enumerate(DEP)]
            S.til.set_validity(by_weight=vbw)
            A.DepositCurrent(S.sheet(api), api.Fields(40, 24, S.g, NCOMP, data=S.slab), S.geom, -1.0, 1.0, order, *comp,
                             n_qsa=cnt, can_ionize=ionize, tiling=S.til, aabs=AABS if laser else -1)
        for order, ts, dt, laser, vbw, _, stale, ionize in EXPL_CASES:
            S = Setup(api, oracle, 40, 24, ts, order, 2, stale, ionize, violators=False)
            S.til.set_validity(by_weight=vbw)
            A.ExplicitDeposition(S.sheet(api), api.Fields(40, 24, S.g, NCOMP, data=S.slab), S.geom, -1.0, 1.0, order, *CACHE,
                                 *SRC, derivative_type=dt, can_ionize=ionize, tiling=S.til, aabs=AABS if laser else -1)
        for order, ts, laser, vbp, (bc, nsub, temp), _, stale, ionize in PUSH_CASES:
            S = Setup(api, oracle, 40, 24, ts, order, 3, stale, ionize, violators=False, bc=bc)
            S.til.set_validity(by_psi_half=vbp)
            A.AdvancePlasmaParticles(S.sheet(api), api.Fields(40, 24, S.g, NCOMP, data=S.slab), S.geom, -1.0, 1.0, order, *PUSH,
                                     temp_slice=temp, n_subcycles=nsub, can_ionize=ionize, tiling=S.til,
                                     aabs=AABS if laser else -1)
        torch.cuda.synchronize()
        for order in ORDERS:
            for ts in TILES:
                for rho in (0, 1):
                    _engine_slices(api, _small_blowout(order, rho, nz=6), ts, 3, fusion=True)
                ion = decks.ionization_SI()
                ion.update(order=order, nx=32, ny=32, nz=6, n_steps=1)
                _engine_slices(api, ion, ts, 3)
                las = decks.laser_ionization_SI()
                las.update(order=order, nz=6, n_steps=1)
                _engine_slices(api, las, ts, 3)
        got = api.recorded_particle_dispatch()
    finally:
        api.record_particle_dispatch(False)
    assert len(EXPECTED) == len(set(EXPECTED)) == 178
    missing, extra = sorted(set(EXPECTED) - got), sorted(got - set(EXPECTED))
    assert not missing and not extra, (missing, extra)
