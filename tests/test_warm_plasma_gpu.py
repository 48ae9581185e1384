"""Warm plasmas on the GPU (u_mean / u_std / temperature_in_ev, do_symmetrize, prevent_centered_particle): the sheets
the engine creates against the numpy restatement (tests/plasma_thermal_reference.py) slot by slot, the zero-key limit, the
neutralising background, the warm symmetrised deck through every particle path at any tiling, the two places that assumed a
plasma at rest (the predictor-corrector's first slice, the ionisable species' tile skip), the symmetry do_symmetrize is there for,
and the refusals.

Tolerances of the sheet comparison: positions to 1e-14 of the box width and weights to a relative 1e-14, as for the fine patch;
momenta |du_d| <= 1e-13 (u_std[d] + |u_mean[d]|): the argument 2 pi u2 and r <= 8.6 bound the error of log / sin / cos near
1e-14 u_std, a factor ten is left for contraction and library differences; psi = sqrt(1 + u.u) - u_z inherits the three
components' bounds (|d sqrt| <= sum |du_d|, plus du_z) and four roundings of gamma."""
import numpy as np
import pytest

from hipace_amd import decks
from tests import plasma_thermal_reference as W
from tests.util import NCOMP, rel_err, smooth_slab

pytestmark = pytest.mark.gpu

SEED = 1
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def short_deck(base=None, nz=20, **kw):
    """the blowout deck around the driver's centre, as tests/test_fine_patch_gpu.py::short_deck, with the warm keys at 0"""
    d = base if base is not None else decks.blowout_wake()
    h = 0.06 * nz
    d.update(nz=nz, n_steps=1, lo=(d["lo"][0], d["lo"][1], -h), hi=(d["hi"][0], d["hi"][1], h), beam_zmin=-h + 0.01, beam_zmax=h - 0.01)
    d.update(decks.PLASMA_INIT_DEFAULT)
    d.update(decks.PLASMA_THERMAL_DEFAULT)
    d.update(plasma_seed=SEED)
    d.update(kw)
    return d


def cell_mask(deck, f):
    nx, ny = deck["nx"], deck["ny"]
    dx, dy = (deck["hi"][0] - deck["lo"][0]) / nx, (deck["hi"][1] - deck["lo"][1]) / ny
    x = deck["lo"][0] + (np.arange(nx) + 0.5) * dx
    y = deck["lo"][1] + (np.arange(ny) + 0.5) * dy
    return np.broadcast_to(np.asarray(f(x[None, :], y[:, None])), (ny, nx)) > 0


def light_speed(deck):
    return 299792458.0 if deck.get("si_units", 0) else 1.0


def restated(deck, species, step=0, patch=None, T=2):
    si = bool(deck.get("si_units", 0))
    fine = tuple(deck[species + "_fine_ppc"])
    use = patch is not None and any(fine)
    return W.init_particles_warm(
        deck["nx"], deck["ny"], deck["lo"], deck["hi"], deck["nz"], tuple(deck[species + "_ppc"]), fine if use else None,
        cell_mask(deck, patch) if use else None, T, density=deck[species + "_density"],
        radius=deck["plasma_radius"] if deck["plasma_radius"] > 0.0 else np.inf,
        hollow_core_radius=deck.get("plasma_hollow_core_radius", 0.0), normalized=not si,
        u_mean=deck[species + "_u_mean"], u_std=decks.thermal_u_std(deck, species), seed=deck["plasma_seed"],
        species=0 if species == "plasma" else 1, step=step, c=light_speed(deck), do_symmetrize=bool(deck["plasmas_do_symmetrize"]),
        prevent_centered_particle=bool(deck["plasmas_prevent_centered_particle"]))


def assert_warm_sheet(real, valid, ref, deck, species, worst=None):
    """the engine's sheet IN SLOT ORDER against the restatement, slot by slot"""
    width, c = deck["hi"][0] - deck["lo"][0], light_speed(deck)
    u_mean, u_std = deck[species + "_u_mean"], decks.thermal_u_std(deck, species)
    assert real.shape[1] == ref["nslots"]
    assert np.array_equal(np.flatnonzero(valid), ref["slot"])
    g = real[:, ref["slot"]]
    ex, ey = np.abs(g[0] - ref["x"]).max() / width, np.abs(g[1] - ref["y"]).max() / width
    ew = np.abs(g[2] / ref["w"] - 1.0).max()
    print(f"sheet: {ref['slot'].size} of {ref['nslots']} slots valid, dx {ex:.2e} dy {ey:.2e} of the width, dw {ew:.2e} relative")
    assert ex <= 1e-14 and ey <= 1e-14 and ew <= 1e-14
    tol = [1e-13 * (u_std[d] + abs(u_mean[d])) for d in range(3)]
    for d in range(2):
        err = np.abs(g[3 + d] / c - ref["u"][d]).max()
        print(f"  u[{d}]: max |du| {err:.2e}, bound {tol[d]:.2e}" + (f" ({err / tol[d] * 1e-13:.2e} of u_std + |u_mean|)" if tol[d] else ""))
        if worst is not None and tol[d]:
            worst.append(err / tol[d] * 1e-13)
        assert err <= tol[d], (d, err, tol[d])
    gamma = np.sqrt(1.0 + (ref["u"] ** 2).sum(axis=0))
    epsi, tpsi = np.abs(g[5] - ref["psi"]).max(), 2.0 * sum(tol) + 4.0 * EPS * gamma.max()
    print(f"  psi: max |dpsi| {epsi:.2e}, bound {tpsi:.2e}")
    assert epsi <= tpsi and g[5].min() > 0.0
    assert np.array_equal(g[6], g[0]) and np.array_equal(g[7], g[1])                                   # x_prev, y_prev
    assert np.array_equal(g[8], g[3]) and np.array_equal(g[9], g[4]) and np.array_equal(g[10], g[5])   # half-step copies
    dead = valid == 0
    assert np.all(real[2][dead] == 0.0) and np.all(real[10][dead] == 0.0)                              # invalid slots


def ions_by_slot(eng):
    """the ion sheet in slot order: the key (the id bits) is the slot, whatever the tile sort did"""
    real, valid, lev, key = eng.ions()
    o = np.argsort(key)
    assert np.array_equal(key[o], np.arange(key.size))
    return real[:, o], valid[o], lev[o]


# ---- 1. the sheet against the restatement -------------------------------------------------------------------------------------

SHEET_CASES = {
    # name: (deck changes, fine patch radius or None, steps)
    "u_std_only": (dict(plasma_u_std=(0.05, 0.05, 0.05)), None, (0, 3)),
    "u_mean_only": (dict(plasma_u_mean=(0.02, -0.03, 0.5)), None, (0,)),
    "anisotropic_ppc2": (dict(plasma_ppc=(2, 2), plasma_u_mean=(0.01, 0.0, -0.2), plasma_u_std=(0.3, 0.0, 0.5)), None, (0, 1)),
    "temperature_symmetrized": (dict(plasma_temperature_in_ev=50.0, plasmas_do_symmetrize=1), None, (0, 2)),
    "patch_radius_hollow_symmetrized": (dict(plasma_fine_ppc=(4, 4), plasma_radius=5.0, plasma_hollow_core_radius=1.0,
                                             plasma_u_std=(0.1, 0.2, 0.0), plasmas_do_symmetrize=1), 2.0, (0,)),
    "patch_radius": (dict(plasma_fine_ppc=(2, 4), plasma_radius=6.0, plasma_u_std=(0.1, 0.1, 0.1)), 2.0, (0, 5)),
    "63x63_prevent_symmetrized": (dict(nx=63, ny=63, plasma_u_std=(0.05, 0.05, 0.05), plasmas_do_symmetrize=1,
                                       plasmas_prevent_centered_particle=1), None, (0,)),
    # (the engine's grids have nx and ny of the same parity: ppc 1 x 2 shifts x only)
    "63x63_prevent_cold_ppc_1x2": (dict(nx=63, ny=63, plasma_ppc=(1, 2), plasmas_prevent_centered_particle=1), None, (0,)),
    "SI_temperature": ("SI", None, (0,)),
}
WORST = []


@pytest.mark.parametrize("case", sorted(SHEET_CASES))
def test_sheet_matches_the_restatement(api, case):
    changes, radius, steps = SHEET_CASES[case]
    if changes == "SI":
        deck = short_deck(decks.blowout_wake_SI(), nz=4, plasma_temperature_in_ev=200.0, plasma_u_mean=(0.0, 0.01, 0.0))
        kp_inv = deck["hi"][0] / 8.0
        deck.update(lo=(deck["lo"][0], deck["lo"][1], -0.24 * kp_inv), hi=(deck["hi"][0], deck["hi"][1], 0.24 * kp_inv),
                    beam_zmin=-0.2 * kp_inv, beam_zmax=0.2 * kp_inv)
    else:
        deck = short_deck(nz=4, **changes)
    patch = decks.fine_patch_disc(radius) if radius else None
    sheets = []
    for step in steps:
        eng = api.SliceEngine(deck, tile_size=0, fine_patch=patch, fine_transition_cells=2)
        eng.set_step(step)
        eng.begin_step()
        real, valid = eng.particles()
        ref = restated(deck, "plasma", step, patch)
        assert eng.nparticles == real.shape[1] == ref["nslots"]
        assert_warm_sheet(real, valid, ref, deck, "plasma", WORST)
        sheets.append(real)
    if WORST:
        print(f"worst |du| / (u_std + |u_mean|) so far: {max(WORST):.2e}")
    if len(sheets) == 2:
        # the positions stay, every draw differs
        assert np.array_equal(sheets[0][:2], sheets[1][:2])
        if any(decks.thermal_u_std(deck, "plasma")):
            live = ref["slot"]
            assert np.all(sheets[0][5][live] != sheets[1][5][live])
    if "prevent" in case:
        live, ppc = valid != 0, deck["plasma_ppc"]
        sx, sy = W.shifts(deck["nx"], deck["ny"], ppc, True)
        assert sx and sy == ("1x2" not in case)
        assert not np.any(real[0][live] == 0.0) and (not sy or not np.any(real[1][live] == 0.0))
        n1 = (deck["nx"] - 1) * (deck["ny"] - 1 if sy else deck["ny"])
        assert live.sum() == n1 * ppc[0] * ppc[1] * (4 if deck["plasmas_do_symmetrize"] else 1)


@pytest.mark.parametrize("tile_size", [0, 16])
def test_ion_sheet_matches_the_restatement(api, tile_size):
    """species 1 has its own link in the chain of the draws, its own u_std (here from its temperature and mass) and fine_ppc; it
    is a keyed species: the id bits carry the slot, mirror copies included"""
    patch = decks.fine_patch_disc(2.0)
    deck = short_deck(nz=4, plasma_fine_ppc=(4, 4), ion_fine_ppc=(2, 2), background_density_SI=1.0e24, plasma_u_std=(0.05, 0.05, 0.05),
                      ion_u_mean=(0.0, 0.001, 0.0), ion_temperature_in_ev=2000.0, plasmas_do_symmetrize=1, plasma_radius=6.0)
    decks.with_ion_species(deck, "H", 1.0, ppc=(1, 1), initial_level=1)
    assert 1e-3 < decks.thermal_u_std(deck, "ion")[0] < 2e-3
    for step in (0, 2):
        eng = api.SliceEngine(deck, tile_size=tile_size, fine_patch=patch, fine_transition_cells=2)
        eng.set_step(step)
        eng.begin_step()
        real, valid, lev = ions_by_slot(eng)
        assert_warm_sheet(real, valid, restated(deck, "ion", step, patch), deck, "ion", WORST)
        assert np.all(lev == 1)
        if tile_size == 0:
            assert_warm_sheet(*eng.particles(), restated(deck, "plasma", step, patch), deck, "plasma", WORST)


# ---- 2. all keys zero: the deck as it was ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["plain", "fine_patch"])
def test_zero_keys_are_the_deck_without_them(api, kind):
    """both setters called with zeros and false: bit-equal sheets, and the first slices' slabs equal to the plain deck's -- bit for
    bit if two runs of the plain deck are, else within ten times what those two runs differ by (the atomics' order)"""
    patch = decks.fine_patch_disc(2.0) if kind == "fine_patch" else None
    deck = short_deck(nz=4, plasma_fine_ppc=(4, 4) if patch else (0, 0))

    def run(zero_keys):
        eng = api.SliceEngine(deck, tile_size=16, sort_period=5, fine_patch=patch, fine_transition_cells=2)
        if zero_keys:
            eng.set_plasma_momentum(0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0)
            eng.set_plasma_symmetry(False, False)
        eng.begin_step()
        sheet = eng.particles()
        for isl in (3, 2, 1):
            eng.solve_slice(isl)
        return sheet, eng.slab()

    (ra, va), sa = run(False)
    (rb, vb), sb = run(False)
    (rz, vz), sz = run(True)
    assert np.array_equal(rz, ra) and np.array_equal(vz, va) and np.array_equal(rb, ra)
    assert np.abs(sa).max() > 0.0
    for c in range(sa.shape[0]):
        noise, diff = np.abs(sa[c] - sb[c]).max(), np.abs(sz[c] - sa[c]).max()
        assert diff <= 10.0 * noise, (c, diff, noise)


# ---- 3. the neutralising background ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile_size", [0, 16])
def test_background_cancels_a_warm_plasma(api, tile_size):
    """rho - jz of a particle is its weight whatever its momentum: on the first solved slice of a deck without a beam the plasma's
    rhomjz on top of the ion background (the plane starts from it) is 0 to 1e-12 of the sum of |w| per cell"""
    from hipace_amd._lib import CIDX
    deck = short_deck(nz=4, beam_profile=-1, plasma_ppc=(3, 3), plasma_u_mean=(0.0, 0.0, 0.3), plasma_u_std=(0.3, 0.2, 0.5),
                      plasmas_do_symmetrize=1)      # (3 x 3: the shape factors of a 2^n lattice are dyadic, their sums exact)
    eng = api.SliceEngine(deck, tile_size=tile_size)
    eng.begin_step()
    real, valid = eng.particles()
    w_cell = real[2][valid != 0].sum() / (deck["nx"] * deck["ny"])
    assert w_cell == pytest.approx(1.0, rel=1e-12)
    eng.solve_slice(deck["nz"] - 1)
    s = eng.slab()
    assert np.abs(s[CIDX["Ion_rhomjz"]]).max() > 0.9 * w_cell
    worst = np.abs(s[CIDX["rhomjz"]]).max()
    print(f"max |rhomjz + background| {worst:.2e} of {w_cell} per cell")
    assert worst <= 1e-12 * w_cell
    assert np.abs(real[3]).max() > 0.9 and np.abs(s[CIDX["chi"]]).max() > 0.5       # the plasma is warm, and deposited


# ---- 4. the warm symmetrised deck through every particle path ------------------------------------------------------------------

def _variant(name):
    if name == "laser":
        d = short_deck(decks.laser_blowout_wake())
        d.update(nx=64, ny=64, lo=(-16.0, -16.0, d["lo"][2]), hi=(16.0, 16.0, d["hi"][2]))
    else:
        d = short_deck()
    d.update(plasma_temperature_in_ev=50.0, plasmas_do_symmetrize=1)
    if name == "predictor_corrector":
        d = decks.predictor_corrector(d)
    elif name in ("ion", "ion_ionizing"):
        d.update(background_density_SI=1.0e24, ion_u_std=(0.02, 0.02, 0.02))
        decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=0 if name == "ion_ionizing" else 1)
        if name == "ion":
            d.update(plasma_no_neutralize=1)
    elif name == "moving_beam":
        d.update(dt=0.9)
    elif name == "collisions":
        d.update(background_density_SI=1.0e24, collisions=[(0, 0, -1.0, 0)])
    return d


@pytest.mark.parametrize("name", ["explicit", "predictor_corrector", "ion", "ion_ionizing", "laser", "moving_beam", "collisions", "fused"])
def test_warm_symmetrized_deck_any_tiling(api, name):
    """one whole step: tile sizes 16 (re-sorted every slice) and 32 (every 7th at the latest) against the per-particle kernels, as
    test_non_uniform_sheet_any_tiling"""
    deck = _variant(name)
    out = {}
    for ts, period in ((0, 1), (16, 1), (32, 7)):
        eng = api.SliceEngine(deck, tile_size=ts, sort_period=period)
        assert eng.nparticles == 4 * 64 * 64
        if name == "fused" and ts:
            eng.set_fusion(True)
        eng.set_diagnostics(True)
        eng.run_step()
        out[ts] = (eng.checksums(), eng.fallbacks(), eng.sorts(), eng.ion_stats() if deck["ion_on"] else None)
        if name == "collisions":
            assert eng.collision_stats()["pairs_collided"] > 0
    ref = out[0][0]
    assert sum(v != 0.0 for v in ref.values()) >= 8
    for ts in (16, 32):
        cs, fallbacks, sorts, ions = out[ts]
        for k, v in ref.items():
            if v != 0.0:
                assert abs(cs[k] - v) <= 1e-9 * abs(v), (ts, k, cs[k], v)
        assert fallbacks >= 0 and sorts > 0
        assert ions == out[0][3]
    assert out[0][1] == 0 and out[0][2] == 0
    if name == "ion_ionizing":
        assert out[0][3][0] > 0
    if name == "ion":
        assert out[0][3][0] == 0


@pytest.mark.parametrize("tile_size", [0, 16])
def test_predictor_corrector_takes_the_warm_currents_from_the_first_slice(api, tile_size):
    """A warm plasma deposits real jx, jy from the first slice on.  Without a beam a cold deck's loop leaves every slice after
    one pass with Bx = By = 0 exactly (nothing but rounding residue has been deposited).  The warm deck's first slice also leaves
    after one pass -- its guess is B = 0, and the relative error of a zero guess is 0 by definition (fields/Fields.cpp:1283), in
    the reference too -- but it keeps the B of its currents, and from the second slice on the loop iterates on it."""
    from hipace_amd._lib import CIDX_PC
    cold = decks.predictor_corrector(short_deck(nz=4, beam_profile=-1))
    warm = decks.predictor_corrector(short_deck(nz=4, beam_profile=-1, plasma_u_std=(0.05, 0.05, 0.05)))
    res = {}
    for key, deck in (("cold", cold), ("warm", warm)):
        eng = api.SliceEngine(deck, tile_size=tile_size)
        eng.begin_step()
        eng.solve_slice(3)
        b1, first = np.abs(eng.slab()[CIDX_PC["Bx"]]).max(), eng.pc_stats()
        eng.solve_slice(2)
        res[key] = (b1, first, eng.pc_stats())
    print("predictor-corrector: (max |Bx| after the first slice, (iterations, error) after it, after the second):", res)
    assert res["cold"][0] == 0.0 and res["cold"][1] == (1, 0.0) and res["cold"][2] == (2, 0.0)
    assert res["warm"][0] > 0.0 and res["warm"][1] == (1, 0.0)
    assert res["warm"][2][0] >= 3 and res["warm"][2][1] > 0.0


@pytest.mark.parametrize("tile_size,driver", [(16, False), (32, False), (16, True)])
def test_warm_neutral_atoms_stream_freely(api, tile_size, driver):
    """Neutral atoms carry no charge: whatever the field, one that is still neutral after n slices sits at x0 + n dz ux / (psi c)
    with the momentum it was created with.  The tile skip of the ionisable species is a bound for atoms AT REST; a warm species
    must not take it.  Without a driver every tile is below the threshold (the skip would hold every atom in place); behind the
    driver the atoms it has not ionised stream on through its field.  Bound: per slice one rounding of the position (|x| < 8) and
    a few ulp of the step, 2 ulp(8) in all."""
    n_slices = 5
    deck = short_deck(background_density_SI=1.0e24, ion_u_mean=(0.01, 0.0, 0.0), ion_u_std=(0.05, 0.05, 0.05),
                      **({} if driver else dict(beam_profile=-1)))
    decks.with_ion_species(deck, "H", 1.0, ppc=(1, 1), initial_level=0)
    dz = (deck["hi"][2] - deck["lo"][2]) / deck["nz"]
    eng = api.SliceEngine(deck, tile_size=tile_size, sort_period=3)
    eng.begin_step()
    r0, v0, lev0 = ions_by_slot(eng)
    assert np.all(lev0 == 0) and np.all(v0 == 1)
    for isl in range(deck["nz"] - 1, deck["nz"] - 1 - n_slices, -1):
        eng.solve_slice(isl)
    r1, v1, lev1 = ions_by_slot(eng)
    # away from the periodic boundary, and still neutral
    far = (np.abs(r0[0]) < 7.5) & (np.abs(r0[1]) < 7.5) & (lev1 == 0) & (v1 == 1)
    assert far.sum() > 3000
    want_x = r0[0].copy()
    want_y = r0[1].copy()
    for _ in range(n_slices):
        want_x = want_x + dz * (r0[3] / r0[5])
        want_y = want_y + dz * (r0[4] / r0[5])
    ex, ey = np.abs(r1[0] - want_x)[far].max(), np.abs(r1[1] - want_y)[far].max()
    moved = np.abs(r1[0] - r0[0])[far]
    print(f"free streaming over {n_slices} slices: max error {max(ex, ey):.2e}, displacements up to {moved.max():.2e}")
    assert moved.min() > 0.0 and moved.max() > 0.03
    assert max(ex, ey) <= n_slices * 2.0 * np.spacing(8.0)
    for q in (3, 4, 5):
        assert np.array_equal(r1[q][far], r0[q][far])


# ---- 5. the operators on a warm sheet against the oracle --------------------------------------------------------------------------

@pytest.mark.parametrize("ts", [16, 32])
def test_tiled_operators_on_a_warm_sheet_vs_oracle(api, oracle, ts):
    deck = short_deck(nz=4, plasma_ppc=(2, 2), plasma_u_mean=(0.0, 0.05, 0.0), plasma_u_std=(0.3, 0.3, 0.3), plasmas_do_symmetrize=1)
    eng = api.SliceEngine(deck, tile_size=0)
    eng.begin_step()
    real, valid = eng.particles()
    assert np.abs(real[3]).max() > 0.9 and real.shape[1] == 16 * 64 * 64
    n, order, g = deck["nx"], deck["order"], (deck["order"] + 1) // 2 + 1
    lo, hi = deck["lo"][:2], deck["hi"][:2]
    ion = np.zeros(real.shape[1], dtype=np.int32)
    geom = api.Geometry(n, n, lo, hi, 0.3)
    ogeom = oracle.make_geom(n, n, lo, hi, dz=0.3, bc=1)
    til = api.Tiling(n, n, ts, real.shape[1])
    sheet = til.reorder(api.PlasmaSheet(real, valid, ion), geom)
    sreal, svalid = sheet.numpy()
    slab = smooth_slab(n, n, g, amp=0.2)

    def fresh():
        return api.PlasmaSheet(sreal, svalid, ion), api.Fields(n, n, g, NCOMP, data=slab)

    ref = slab.copy()
    comp = [15, 16, -1, 18, 2, 17]
    oracle.deposit_current(ref, n, n, g, sreal.copy(), svalid.copy(), ion, ogeom, comp, -1.0, 1.0, order)
    pl, f = fresh()
    til.fallback.zero_()
    api.DepositCurrent(pl, f, geom, -1.0, 1.0, order, jx=15, jy=16, rho=18, chi=2, rhomjz=17, tiling=til)
    out = f.numpy()
    for c in (15, 16, 18, 2, 17):
        assert rel_err(out[c] - slab[c], ref[c] - slab[c]) < 1e-12, c
    assert til.fallback.item() == 0

    ref = slab.copy()
    oracle.explicit_deposit(ref, n, n, g, sreal.copy(), svalid.copy(), ion, ogeom, [10, 7, 5, 6], [3, 4], -1.0, 1.0, order, 2)
    pl, f = fresh()
    api.ExplicitDeposition(pl, f, geom, -1.0, 1.0, order, Bz=10, Ez=7, ExmBy=5, EypBx=6, Sy=3, Sx=4, tiling=til)
    out = f.numpy()
    for c in (3, 4):
        assert rel_err(out[c] - slab[c], ref[c] - slab[c]) < 1e-12, c

    r2, v2 = sreal.copy(), svalid.copy()
    oracle.advance_plasma(slab, n, n, g, r2, v2, ion, ogeom, [11, 7, 8, 9, 10], -1.0, 1.0, order)
    pl, f = fresh()
    api.AdvancePlasmaParticles(pl, f, geom, -1.0, 1.0, order, Psi=11, Ez=7, Bx=8, By=9, Bz=10, tiling=til)
    greal, gvalid = pl.numpy()
    assert np.array_equal(gvalid, v2)
    live = v2 != 0
    for k in range(11):
        assert rel_err(greal[k][live], r2[k][live]) < 1e-10, k


# ---- 6. symmetry ------------------------------------------------------------------------------------------------------------

def asymmetry(plane, odd_x=False, odd_y=False):
    """max |F - (+-) its mirror image in x, in y| / max |F| over the cells of the box"""
    fx = plane[:, ::-1] * (-1.0 if odd_x else 1.0)
    fy = plane[::-1, :] * (-1.0 if odd_y else 1.0)
    return max(np.abs(plane - fx).max(), np.abs(plane - fy).max()) / max(np.abs(plane).max(), 1e-300)


@pytest.mark.parametrize("grid", [64, 63])
def test_sources_of_the_symmetrized_sheet_are_symmetric(api, grid):
    """jx odd in x, jy odd in y, rhomjz and chi even, deposited from the fresh sheet: to 1e-12 of each plane's maximum"""
    deck = short_deck(nz=4, nx=grid, ny=grid, plasma_ppc=(1, 1), plasma_u_std=(0.1, 0.1, 0.1), plasmas_do_symmetrize=1,
                      plasmas_prevent_centered_particle=int(grid == 63))
    eng = api.SliceEngine(deck, tile_size=0)
    eng.begin_step()
    real, valid = eng.particles()
    n, order, g = grid, deck["order"], (deck["order"] + 1) // 2 + 1
    geom = api.Geometry(n, n, deck["lo"][:2], deck["hi"][:2], 0.12)
    for ts in (0, 16):
        ion = np.zeros(real.shape[1], dtype=np.int32)
        til = api.Tiling(n, n, ts, real.shape[1]) if ts else None
        sheet = api.PlasmaSheet(real, valid, ion)
        if til is not None:
            sheet = til.reorder(sheet, geom)
        f = api.Fields(n, n, g, NCOMP, data=np.zeros((NCOMP, n + 2 * g, n + 2 * g)))
        api.DepositCurrent(sheet, f, geom, -1.0, 1.0, order, jx=15, jy=16, rho=18, chi=2, rhomjz=17, **({"tiling": til} if til else {}))
        out = f.numpy()[:, g:-g, g:-g]
        res = {"jx": asymmetry(out[15], odd_x=True), "jy": asymmetry(out[16], odd_y=True), "rhomjz": asymmetry(out[17]), "chi": asymmetry(out[2])}
        print(f"grid {grid} tile {ts}: asymmetry of the source planes {res}")
        assert np.abs(out[15]).max() > 1e-3
        for k, v in res.items():
            assert v <= 1e-12, (k, v)


def test_symmetrized_warm_wake_stays_symmetric(api):
    """10 slices behind the deck's symmetric driver (fixed ppc on the grid): Ez and Psi are even, ExmBy is odd in x and even in y.
    The cold deck runs the untouched path and shows the solver's own asymmetry; the symmetrised warm deck stays within ten
    times that; the unsymmetrised warm deck is the contrast."""
    from hipace_amd._lib import CIDX
    u = (0.03, 0.03, 0.03)
    cases = {"cold": short_deck(nz=10), "warm_symmetrized": short_deck(nz=10, plasma_u_std=u, plasmas_do_symmetrize=1),
             "warm": short_deck(nz=10, plasma_u_std=u)}
    res = {}
    for key, deck in cases.items():
        eng = api.SliceEngine(deck, tile_size=16)
        eng.run_step()
        g = eng.ng
        s = eng.slab()[:, g:-g, g:-g]
        res[key] = {"Ez": asymmetry(s[CIDX["Ez"]]), "Psi": asymmetry(s[CIDX["Psi"]]), "ExmBy": asymmetry(s[CIDX["ExmBy"]], odd_x=True)}
    print("asymmetry after 10 slices:", res)
    for k in ("Ez", "Psi", "ExmBy"):
        assert res["warm_symmetrized"][k] <= 10.0 * res["cold"][k], (k, res)
        assert res["warm"][k] > res["warm_symmetrized"][k], (k, res)


# ---- 7. refusals, counts -------------------------------------------------------------------------------------------------------

def test_refusals(api):
    def fails(fn, needle):
        with pytest.raises(RuntimeError) as ei:
            fn()
        assert needle in str(ei.value), str(ei.value)

    base = short_deck(nz=4)
    mask = np.ones((64, 64), bool)
    zero = (0.0, 0.0, 0.0)
    fails(lambda: api.SliceEngine(dict(base, plasma_u_std=(0.1, -0.1, 0.1))), "u_std must not be negative")
    fails(lambda: api.SliceEngine(dict(base, ion_u_std=(0.1, 0.1, 0.1))), "does not have this species")
    fails(lambda: api.SliceEngine(base).set_plasma_momentum(2, zero, zero, 0), "species must be 0")
    with pytest.raises(ValueError, match="exclusively"):
        api.SliceEngine(dict(base, plasma_u_std=(0.1, 0.1, 0.1), plasma_temperature_in_ev=10.0))
    # prevent_centered_particle with the fine patch: whichever comes second
    odd = dict(base, nx=63, ny=63)
    fails(lambda: api.SliceEngine(dict(odd, plasma_fine_ppc=(4, 4), plasmas_prevent_centered_particle=1)), "prevent_centered_particle cannot")
    eng = api.SliceEngine(dict(odd, plasmas_prevent_centered_particle=1))
    fails(lambda: eng.set_fine_patch(np.ones((63, 63), bool), 2), "prevent_centered_particle cannot")
    eng = api.SliceEngine(odd, fine_patch=np.ones((63, 63), bool))
    fails(lambda: eng.set_plasma_symmetry(False, True), "prevent_centered_particle cannot")
    eng.set_plasma_symmetry(True, False)                       # do_symmetrize alone goes with the patch
    # after the first begin_step
    eng = api.SliceEngine(base)
    eng.begin_step()
    fails(lambda: eng.set_plasma_momentum(0, zero, (0.1, 0.1, 0.1), 0), "before the first hps_engine_begin_step")
    fails(lambda: eng.set_plasma_symmetry(True, False), "before the first hps_engine_begin_step")


@pytest.mark.parametrize("order", ["tiling_first", "symmetry_first"])
def test_counts_follow_the_mirror_copies(api, order):
    """hps_engine_info, the sheets and the tiling capacity: four times the sheet, fine patch and released electrons included"""
    patch = decks.fine_patch_disc(2.0)
    deck = short_deck(nz=4, plasma_fine_ppc=(4, 4), ion_fine_ppc=(2, 2), background_density_SI=1.0e24, plasma_u_std=(0.01, 0.01, 0.01))
    decks.with_ion_species(deck, "H", 1.0, ppc=(1, 1), initial_level=0)
    ncell = int(cell_mask(deck, patch).sum())
    plain = api.SliceEngine(deck, fine_patch=patch, fine_transition_cells=0)
    assert plain.nparticles == 64 * 64 + 15 * ncell
    eng = api.SliceEngine(deck)
    if order == "tiling_first":
        eng.set_tiling(32, 3)
        eng.set_plasma_symmetry(True, False)
        eng.set_fine_patch(patch, 0)
    else:
        eng.set_plasma_symmetry(True, False)
        eng.set_fine_patch(patch, 0)
        eng.set_tiling(32, 3)
    assert eng.nparticles == 4 * plain.nparticles
    eng.begin_step()
    real, valid = eng.particles()
    ireal, ivalid, _, key = eng.ions()
    assert real.shape[1] == 4 * plain.nparticles and valid.sum() == real.shape[1]
    assert ireal.shape[1] == 4 * (64 * 64 + 3 * ncell) and sorted(key) == list(range(ireal.shape[1]))
    assert real[2].sum() == pytest.approx(64 * 64, rel=1e-13)
    eng.solve_slice(deck["nz"] - 1)
    assert eng.sorts() > 0
