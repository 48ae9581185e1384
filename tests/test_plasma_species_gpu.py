"""Further plasma species in one engine (hps_engine_add_plasma_species) on the GPU.  The oracle knows two species, so
the pins are equivalences that hold by construction -- a split population is one population, a heavy species is the
neutralising background, slot 1 and slot 2 give the same ions, the order of addition does not matter -- plus the numpy
restatements of the warm draws and of the collisions, the three-species deck, the refusals, and the untouched engine."""
import numpy as np
import pytest

from hipace_amd import _lib, decks
from tests import collision_reference as CR
from tests import plasma_thermal_reference as TR

pytestmark = pytest.mark.gpu

# ---- the bound of the equivalences ---------------------------------------------------------------------------------------
# Two runs of ONE deck that differ only in the order of the depositions' sums (tile size 16 against 32, and 0 against 16),
# measured on the commit before this feature on the MI355X: per field component the largest |difference| over all 24 slices
# divided by the component's largest magnitude, the largest over the components FIELDS and over the grids 64 x 64 and 48 x 80.
#   explicit solver (the deck of equivalences 1, 2 and 4):      8.01e-14 (Bz, 64 x 64, tile 0 against 16; 16 against 32: 1.14e-14)
#   predictor-corrector (equivalence 2 under the loop):          1.48e-14 (Bz, 64 x 64, tile 0 against 16), 162 iterations in every run
#   the mobile-ion deck (equivalence 3):                         2.25e-14 (Bz, 64 x 64, tile 0 against 16)
# (Bz nearly vanishes by symmetry, so its rounding weighs most against its own magnitude; Psi, Ez, ExmBy, EypBx, Bx, By: 5e-16 .. 1e-14.)
# The bound is 100 x that: two sheets differ more in summation order than two tilings, and the wake feeds back over 24 slices.
MEASURED_EXPLICIT = 8.01e-14
MEASURED_PC = 1.48e-14
MEASURED_ION = 2.25e-14
FACTOR = 100.0
NEGATIVE_CONTROL = 1.0e-2      # engine B without its further species differs from A by more than this on Ez

FIELDS = ("Psi", "Ez", "Bz", "ExmBy", "EypBx", "Bx", "By")
GRIDS = {"64x64_t16": (64, 64, 16), "48x80_t32": (48, 80, 32), "64x64_t0": (64, 64, 0)}
OPERATOR_BOUND = 3.8e-13       # tests/test_collisions_gpu.py: engine or operator against tests/collision_reference.py
from tests.test_collisions_cpu import CONSERVATION_BOUND      # noqa: E402  (the two-species conservation check's bound)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import api as A
    _lib.lib()
    return A


# ---- decks -----------------------------------------------------------------------------------------------------------------
def base_deck(nx=64, ny=64, **kw):
    """the blowout wake on nx x ny cells, 24 slices around the middle of its static Gaussian driver (the driver covers every
    slice), electrons 2 x 2 per cell, explicit solver"""
    d = decks.blowout_wake()
    d.update(nx=nx, ny=ny, nz=24, n_steps=1, lo=(-8.0, -8.0, -1.44), hi=(8.0, 8.0, 1.44), plasma_ppc=(2, 2))
    d.update(kw)
    return d


def ion_deck(nx=64, ny=64, further=False, **kw):
    """electrons without a background and mobile hydrogen ions of 5 electron masses at their top level, one per cell: as species
    1 ("ion", ion_init_level = ion_Z = 1: the ion_lev path) or, further=True, as further species 2 (the fixed-charge path)"""
    d = base_deck(nx, ny, plasma_no_neutralize=1, background_density_SI=1.0e24)
    if further:
        d["plasma_species"] = [dict(name="H", charge=1.0, mass=5.0, density=1.0, ppc=(1, 1), neutralize_background=False)]
    else:
        decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=1)
        d["ion_mass"] = 5.0
    d.update(kw)
    return d


def unsplit_decks(nx, ny):
    """the decks whose summation-order noise sets the bounds (measured on the commit before the feature: profiles/plasma_species.txt)"""
    return dict(explicit=base_deck(nx, ny), pc=decks.predictor_corrector(base_deck(nx, ny)), ion=ion_deck(nx, ny))


def run_slices(api, deck, tile_size, species=(), before_step=None):
    """-> (engine, {field: (nz, ny + 2g, nx + 2g)}) of one step, every slice's planes as the slice leaves them"""
    e = api.SliceEngine(deck, tile_size=tile_size)
    for s in species:
        e.add_plasma_species(**s)
    if before_step:
        before_step(e)
    names = _lib.COMPS_PC if deck.get("bxby_solver", 0) else _lib.COMPS
    out = {f: [] for f in FIELDS}
    e.begin_step()
    for isl in range(deck["nz"] - 1, -1, -1):
        e.solve_slice(isl)
        slab = e.slab()
        for f in FIELDS:
            out[f].append(slab[names.index(f)].copy())
    return e, {f: np.stack(v) for f, v in out.items()}


def deviation(a, b):
    """{field: max |a - b| over the box / max |a|}"""
    return {f: float(np.abs(a[f] - b[f]).max() / max(np.abs(a[f]).max(), 1e-300)) for f in FIELDS}


def check_equivalence(name, A, B, B_without, measured):
    for f in FIELDS:
        assert np.isfinite(A[f]).all() and np.isfinite(B[f]).all(), (name, f)
    dev = deviation(A, B)
    ctl = deviation(A, B_without)["Ez"] if B_without is not None else None
    print(f"{name}: deviation {dev} bound {FACTOR * measured:.3e} negative control Ez {ctl}")
    if ctl is not None:
        assert ctl > NEGATIVE_CONTROL, (name, ctl)
    assert max(dev.values()) <= FACTOR * measured, (name, dev, FACTOR * measured)


_A = {}


def unsplit(api, kind, grid):
    """engine A of the equivalences, run once per kind and grid"""
    if (kind, grid) not in _A:
        nx, ny, ts = GRIDS[grid]
        _A[(kind, grid)] = run_slices(api, unsplit_decks(nx, ny)[kind], ts)
    return _A[(kind, grid)]


# ---- 1. a split population is one population ----------------------------------------------------------------------------------
HALF = dict(name="half", charge=-1.0, mass=1.0, density=0.5, ppc=(2, 2), neutralize_background=True)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_split_population_is_one_population(api, grid):
    nx, ny, ts = GRIDS[grid]
    _, A = unsplit(api, "explicit", grid)
    half = base_deck(nx, ny, plasma_density=0.5)
    eB, B = run_slices(api, half, ts, [HALF])
    _, B0 = run_slices(api, half, ts)
    assert eB.plasma_species() == (["plasma", "ion", "half"], [4 * nx * ny, 0, 4 * nx * ny])
    check_equivalence("split " + grid, A, B, B0, MEASURED_EXPLICIT)


# ---- 2. a heavy species is the neutralising background ----------------------------------------------------------------------------
HEAVY = dict(name="heavy", charge=1.0, mass=1.0e30, density=1.0, ppc=(2, 2), neutralize_background=False)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_heavy_species_is_the_neutralising_background(api, grid):
    nx, ny, ts = GRIDS[grid]
    _, A = unsplit(api, "explicit", grid)
    bare = base_deck(nx, ny, plasma_no_neutralize=1)
    _, B = run_slices(api, bare, ts, [HEAVY])
    _, B0 = run_slices(api, bare, ts)
    check_equivalence("heavy " + grid, A, B, B0, MEASURED_EXPLICIT)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_heavy_species_under_the_predictor_corrector(api, grid):
    nx, ny, ts = GRIDS[grid]
    eA, A = unsplit(api, "pc", grid)
    bare = decks.predictor_corrector(base_deck(nx, ny, plasma_no_neutralize=1))
    eB, B = run_slices(api, bare, ts, [HEAVY])
    _, B0 = run_slices(api, bare, ts)
    check_equivalence("heavy pc " + grid, A, B, B0, MEASURED_PC)
    print(f"iterations A {eA.pc_stats()[0]} B {eB.pc_stats()[0]}")
    assert eA.pc_stats()[0] == eB.pc_stats()[0]


# ---- 3. slot 1 and slot 2 give the same ions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_slot_1_and_slot_2_give_the_same_ions(api, grid):
    nx, ny, ts = GRIDS[grid]
    _, A = unsplit(api, "ion", grid)
    _, B = run_slices(api, ion_deck(nx, ny, further=True), ts)                                    # (the deck's own entry)
    _, B0 = run_slices(api, dict(ion_deck(nx, ny, further=True), plasma_species=[]), ts)
    check_equivalence("slots " + grid, A, B, B0, MEASURED_ION)


# ---- 4. order of addition ---------------------------------------------------------------------------------------------------------
LIGHT = dict(name="light", charge=1.0, mass=5.0, density=0.6, ppc=(1, 1), neutralize_background=False)
DENSE = dict(name="dense", charge=1.0, mass=50.0, density=0.4, ppc=(2, 2), neutralize_background=False)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_order_of_addition(api, grid):
    nx, ny, ts = GRIDS[grid]
    bare = base_deck(nx, ny, plasma_no_neutralize=1)
    eA, A = run_slices(api, bare, ts, [LIGHT, DENSE])
    eB, B = run_slices(api, bare, ts, [DENSE, LIGHT])
    _, B0 = run_slices(api, bare, ts, [DENSE])
    assert eA.plasma_species()[0][2:] == ["light", "dense"] and eB.plasma_species()[0][2:] == ["dense", "light"]
    check_equivalence("order " + grid, A, B, B0, max(MEASURED_EXPLICIT, MEASURED_ION))


# ---- 5. per-species state ------------------------------------------------------------------------------------------------------------
def _circle(x, y):
    return x * x + y * y < 9.0


INIT_CASES = {
    "plain": dict(),
    "fine_ppc": dict(fine_ppc=(4, 4)),
    "warm": dict(u_mean=(0.01, 0.0, -0.02), u_std=(0.02, 0.03, 0.01), seed=11),
    "density_expr": dict(density_expr="n0*(1 + 0.05*x)*if(x*x + y*y < 36, 1, 0)", density_constants=dict(n0=0.7), min_density=0.1),
}


@pytest.mark.parametrize("case", sorted(INIT_CASES))
def test_further_species_sheet_is_species_0s_sheet(api, case):
    """species 2 with the parameters of species 0: positions and weights bit for bit; the momenta against the numpy restatement
    of the draws with the species' index (2) in the key"""
    k = INIT_CASES[case]
    deck = base_deck(48, 40, nz=4, plasma_density=0.7)
    if "fine_ppc" in k:
        deck.update(plasma_fine_ppc=k["fine_ppc"], fine_patch=_circle, fine_transition_cells=2)
    if "u_std" in k:
        deck.update(plasma_u_mean=k["u_mean"], plasma_u_std=k["u_std"], plasma_seed=k["seed"])
    if "density_expr" in k:
        deck.update(plasma_density_expr=k["density_expr"], density_constants=k["density_constants"], plasma_min_density=k["min_density"])
    e = api.SliceEngine(deck, tile_size=0)
    idx = e.add_plasma_species(name="twin", charge=-1.0, mass=1.0, density=0.7, ppc=(2, 2), **k)
    assert idx == 2
    e.begin_step()
    r0, v0 = e.particles()
    r2, v2, lev2, _ = e.plasma(species="twin")
    assert r2.shape == r0.shape and r0.shape[1] > 0 and np.array_equal(v0, v2) and v2.sum() > 0
    assert (lev2 == 0).all()
    for q in (0, 1, 2, 6, 7):                      # x, y, w, x_prev, y_prev
        assert np.array_equal(r0[q], r2[q]), (case, q)
    if "u_std" not in k:
        for q in (3, 4, 5, 8, 9, 10):
            assert np.array_equal(r0[q], r2[q]), (case, q)
        return
    slots = np.arange(r2.shape[1])
    for species, r in ((0, r0), (2, r2)):
        _, ux, uy, psi = TR.momenta(slots, k["u_mean"], k["u_std"], k["seed"], species, 0)
        for q, ref in ((3, ux), (4, uy), (5, psi), (8, ux), (9, uy), (10, psi)):
            assert np.abs(r[q] - ref).max() <= 1e-13, (case, species, q, np.abs(r[q] - ref).max())
    assert np.abs(r0[3] - r2[3]).max() > 1e-3      # another species, other draws


def test_insitu_of_the_split_engine(api):
    nx, ny, ts = GRIDS["64x64_t16"]
    e, _ = run_slices(api, base_deck(nx, ny, plasma_density=0.5), ts, [HALF], before_step=lambda e: e.set_insitu_plasma())
    a, b = e.insitu_plasma(species=0), e.insitu_plasma(species="half")
    assert a["sum(w)"].min() > 0.0 and np.array_equal(a["Np"], b["Np"])
    worst = 0.0
    for name in a:
        # a first moment [q] vanishes by symmetry and holds rounding only: its scale is the width sqrt([q^2])
        second = name[:-1] + "^2]"
        scale = np.sqrt(np.abs(a[second]).max()) if second in a and not name.endswith("^2]") else np.abs(a[name]).max()
        worst = max(worst, np.abs(a[name] - b[name]).max() / max(scale, 1e-300))
    print(f"in-situ moments of the two halves: {worst:.3e}")
    assert worst <= FACTOR * MEASURED_EXPLICIT


# ---- 6. collisions ----------------------------------------------------------------------------------------------------------------------
def _sheet(api, e, species):
    real, valid, lev, key = e.plasma(species=species)
    return CR.make_sheet(real[0], real[1], real[2], real[8], real[9], real[10], key=key, ion_lev=lev, valid=valid)


def _collision_engines(api):
    """two engines on warm sheets (species 0 and a further species 2), one of which collides them; one slice"""
    deck = dict(decks.blowout_wake(), nx=16, ny=16, nz=4, n_steps=1, lo=(-2.0, -2.0, -0.24), hi=(2.0, 2.0, 0.24), plasma_ppc=(2, 2),
                beam_profile=-1, background_density_SI=1.0e28, plasma_u_std=(0.05, 0.05, 0.05), plasma_seed=3)
    out = []
    for collide in (True, False):
        e = api.SliceEngine(deck, tile_size=0)
        # (equal weights on both sides: the scheme conserves pair by pair only where no partner is rejected)
        e.add_plasma_species(name="pos", charge=1.0, mass=4.0, density=1.0, ppc=(2, 2), u_std=(0.01, 0.01, 0.01), seed=5)
        if collide:
            e.add_collision("plasma", 2, -1.0, 42)
        e.begin_step()
        e.solve_slice(deck["nz"] - 1)
        out.append(e)
    return deck, out[0], out[1]


def test_collision_with_a_further_species_against_the_restatement(api):
    deck, with_c, without = _collision_engines(api)
    assert with_c.collision_stats()["pairs_collided"] > 200
    a, b = _sheet(api, without, 0), _sheet(api, without, 2)
    ka, kb = _sheet(api, with_c, 0)["key"], _sheet(api, with_c, 2)["key"]
    # tile size 0 keeps the lattice order: the colliding engine's keys are the particle indices, for both species
    assert np.array_equal(ka, np.arange(len(ka))) and np.array_equal(kb, np.arange(len(kb)))
    a["key"], b["key"] = ka, kb
    a0, b0 = CR.copy_sheet(a), CR.copy_sheet(b)
    dx = (deck["hi"][0] - deck["lo"][0]) / deck["nx"]
    dz = (deck["hi"][2] - deck["lo"][2]) / deck["nz"]
    log = CR.collide(a, b, deck["nx"], deck["ny"], deck["lo"][:2], dx, dx, dz, -1.0, 1.0, 1.0, 4.0, coulomb_log=-1.0,
                     background_density_SI=deck["background_density_SI"], normalized=True, seed=42, collision=0, step=0,
                     islice=deck["nz"] - 1)
    assert log["pairs"] == with_c.collision_stats()["pairs_collided"]
    worst = 0.0
    for ref, before, sp in ((a, a0, 0), (b, b0, 2)):
        got = _sheet(api, with_c, sp)
        rms = np.sqrt((before["ux"] ** 2 + before["uy"] ** 2).mean())
        for q in ("ux", "uy", "psi"):
            worst = max(worst, np.abs(got[q] - ref[q]).max() / rms)
        assert np.abs(got["ux"] - before["ux"]).max() > 1e-6 * rms      # the collision did something to this species
    print(f"engine against the numpy restatement: {worst:.3e}")
    assert worst <= OPERATOR_BOUND


def test_collision_with_a_further_species_conserves(api):
    deck, with_c, without = _collision_engines(api)
    totals = []
    for e in (without, with_c):
        p = np.zeros(3)
        en = 0.0
        for sp, m in ((0, 1.0), (2, 4.0)):
            s = _sheet(api, e, sp)
            live = (s["valid"] != 0) & (s["w"] != 0.0)
            ux, uy, psi, w = s["ux"][live], s["uy"][live], s["psi"][live], s["w"][live]
            gamma = (1.0 + ux * ux + uy * uy + psi * psi) / (2.0 * psi)
            uz = gamma - psi
            p += m * np.array([(w * ux).sum(), (w * uy).sum(), (w * uz).sum()])
            en += m * (w * gamma).sum()
            scale_p = m * (w * np.sqrt(ux * ux + uy * uy + uz * uz)).sum()
        totals.append((p, en, scale_p))
    (p0, e0, sc), (p1, e1, _) = totals
    ep, ee = np.abs(p1 - p0).max() / sc, abs(e1 - e0) / e0
    print(f"momentum {ep:.3e} energy {ee:.3e}")
    assert ep <= CONSERVATION_BOUND and ee <= CONSERVATION_BOUND


# ---- 7. three species -------------------------------------------------------------------------------------------------------------------
def test_three_species_deck(api):
    deck = decks.blowout_wake_three_species()
    assert (deck["nx"], deck["ny"], deck["nz"]) == (64, 64, 24)
    e = api.SliceEngine(deck, tile_size=16)
    names, counts0 = e.plasma_species()
    assert names == ["plasma", "ion", "H_ion"] and counts0 == [64 * 64, 64 * 64, 64 * 64]
    rho, g = _lib.CIDX["rho"], e.ng
    dz = (deck["hi"][2] - deck["lo"][2]) / deck["nz"]
    e.begin_step()
    ahead = 0
    for isl in range(deck["nz"] - 1, -1, -1):
        e.solve_slice(isl)
        slab = e.slab()
        assert np.isfinite(slab).all(), isl
        if deck["lo"][2] + isl * dz > deck["beam_zmax"] + dz:       # ahead of the driver: electrons and hydrogen ions cancel
            ahead += 1
            assert np.abs(slab[rho][g:-g, g:-g]).max() <= 1e-12 * deck["plasma_density"], isl
    assert ahead >= 2
    n_ionized, n_plasma = e.ion_stats()
    _, counts = e.plasma_species()
    print(f"ionised {n_ionized}, electrons {n_plasma}")
    assert counts[0] == n_plasma == 64 * 64 + n_ionized and counts[1:] == [64 * 64, 64 * 64]


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
GOOD = dict(charge=1.0, mass=10.0, density=1.0, ppc=(1, 1))


def test_refusals_leave_the_engine_usable(api):
    from hipace_amd._lib import HpsError
    deck = base_deck(32, 32, nz=4)
    e = api.SliceEngine(deck, tile_size=16)

    def refused(engine, status, text, **spec):
        with pytest.raises(HpsError) as err:
            engine.add_plasma_species(**dict(GOOD, **spec))
        assert f"status {status}:" in str(err.value) and text in str(err.value), str(err.value)

    refused(e, 1, "ppc must be >= 1", ppc=(0, 1))
    refused(e, 1, "density must be positive", density=0.0)
    refused(e, 1, "density must be positive", density=-1.0)
    refused(e, 1, "mass must be positive", mass=0.0)
    refused(e, 1, "charge must not be 0", charge=0.0)
    refused(e, 1, "divisible by ppc", ppc=(2, 2), fine_ppc=(3, 4))
    assert e.plasma_species() == (["plasma", "ion"], [4 * 32 * 32, 0])
    for k in range(4):
        assert e.add_plasma_species(**GOOD) == 2 + k
    refused(e, 1, "at most HPS_MAX_PLASMA_SPECIES")
    with pytest.raises(HpsError) as err:
        e.add_beam_collision(2, -1.0, 0)
    assert "status 7:" in str(err.value) and "further plasma species" in str(err.value)
    e.run_step()
    refused(e, 1, "before the first hps_engine_begin_step")
    assert np.isfinite(e.slab()).all() and e.plasma_species()[1] == [4 * 32 * 32, 0] + [32 * 32] * 4
    # SALAME drives the electrons alone: the static beam's and the moving beam's
    s = api.SliceEngine(dict(decks.salame_grid_current(), nx=32, ny=32, nz=8), tile_size=16)
    refused(s, 7, "SALAME")
    m = api.SliceEngine(dict(decks.salame_grid_current_moving(), nx=32, ny=32, nz=8, beam_species_salame=1), tile_size=16)
    refused(m, 7, "SALAME")
    for eng in (s, m):
        eng.begin_step()
        eng.solve_slice(7)
        assert np.isfinite(eng.slab()).all()


# ---- 9. no species added, nothing changed ---------------------------------------------------------------------------------------------------
def test_untouched_engine_is_bit_identical(api):
    """Engines on one deck; one of them asks the new accessors (and is refused a species), the others call nothing new.  Two
    runs of one schedule on tiles may differ by the order of their LDS atomics (tests/test_early_init.py), so two untouched
    runs are compared first: where they agree bit for bit the third must too; otherwise that file's bound for two runs of one
    schedule (1e-12 of the component's largest magnitude) is asserted in its place."""
    deck = base_deck(64, 64, nz=8)
    slabs = []
    for poke in (False, False, True):
        e = api.SliceEngine(deck, tile_size=16)
        if poke:
            assert e.plasma_species()[0] == ["plasma", "ion"]
            with pytest.raises(_lib.HpsError):
                e.add_plasma_species(**dict(GOOD, density=0.0))
        planes = []
        e.begin_step()
        for isl in range(deck["nz"] - 1, -1, -1):
            e.solve_slice(isl)
            planes.append(e.slab())
        slabs.append(np.stack(planes))
        assert e.stats()["early_init"] > 0      # the fast schedule is still the one that runs
    if np.array_equal(slabs[0], slabs[1]):
        assert np.array_equal(slabs[0], slabs[2])
    else:
        print("two untouched runs differ in rounding: asserting the bound of two runs of one schedule")
        for c in range(slabs[0].shape[1]):
            assert np.abs(slabs[0][:, c] - slabs[2][:, c]).max() <= 1e-12 * np.abs(slabs[0][:, c]).max(), c
    # ... and an engine that does hold a further species leaves the fast schedule
    e = api.SliceEngine(deck, tile_size=16)
    e.add_plasma_species(**GOOD)
    e.run_step()
    assert e.stats()["early_init"] == 0


# ---- 10. the laser's initial chi sums every species ------------------------------------------------------------------------------------------
def test_laser_initial_chi_sums_every_species(api):
    """SetInitialChi with further species (tests/test_density_expr_gpu.py::test_laser_initial_chi's box: a 48 x 40 laser grid on
    twice the 24 x 20 field box).  Off the field box shrunk by the guard width laser_chi() is chi_initial as it is:
    sum over the species of n_s(x, y) q_s^2 mu0 / m_s inside the radius, 0 beyond -- species 0 constant, species 1 a program, species
    2 constant, species 3 a program -- to that test's 5e-15."""
    from tests import density_expr_reference as D
    from tests import laser_grid_reference as LG
    d = decks.laser_blowout_wake()
    d.update(nx=24, ny=20, nz=4, lo=(-6.0, -5.0, -0.6), hi=(6.0, 5.0, 0.6), laser_a0=0.5, laser_lambda0=0.4, dt=5.0, n_steps=1,
             laser_solver=1, plasma_radius=5.0, background_density_SI=1.0e24,
             laser_n_cell=(48, 40), laser_patch_lo=(-12.0, -10.0, -0.6), laser_patch_hi=(12.0, 10.0, 0.6), laser_interp_order=1)
    decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=1)
    pi, p3 = "2 - 0.1*y", "0.5 + 0.02*x*x"
    d["ion_density_expr"] = pi
    d["plasma_species"] = [dict(name="He", charge=2.0, mass=7000.0, density=0.3, ppc=(1, 1)),
                           dict(name="warm", charge=-1.0, mass=1.0, density=0.5, ppc=(1, 1), density_expr=p3)]
    lg = decks.laser_geometry(d)[6:]
    with_more = api.SliceEngine(d, tile_size=0)
    without = api.SliceEngine(dict(d, plasma_species=[]), tile_size=0)
    x, y, _ = with_more.laser_cell_centres()
    X, Y = np.meshgrid(x, y)
    g, names = with_more.ng, with_more.comp_names()
    xoff, yoff = LG.pos_offset(-6.0, 6.0, 0.5, 0, 23), LG.pos_offset(-5.0, 5.0, 0.5, 0, 19)
    two = 1.0 * (d["plasma_charge"] ** 2 / d["plasma_mass"]) + D.host_value(pi, X, Y, 0.0) * (d["ion_charge"] ** 2 / d["ion_mass"])
    more = 0.3 * (2.0 ** 2 / 7000.0) + D.host_value(p3, X, Y, 0.0) * 1.0
    got = {}
    for name, eng, want in (("two", without, two), ("four", with_more, two + more)):
        want = np.where(X * X + Y * Y > 25.0, 0.0, want)
        eng.begin_step()
        eng.solve_slice(d["nz"] - 1)
        _, inside = LG.interp_chi(eng.slab()[names.index("chi")], want, lg, 24, 20, g, 0.5, 0.5, xoff, yoff, g, 1)
        off = ~inside
        got[name] = eng.laser_chi()
        assert (off & (want != 0.0)).sum() >= 8 and (off & (want == 0.0)).sum() > 100
        err = np.abs(got[name][off] - want[off]).max() / np.abs(want[off]).max()
        print(f"{name} species: initial chi off the field box to {err:.2e}")
        assert err <= 5e-15 and np.all(got[name][off & (want == 0.0)] == 0.0)
    assert np.abs(got["four"] - got["two"]).max() > 0.1      # the further species weigh in
