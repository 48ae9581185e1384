"""The plasma fine patch (fine_ppc, fine_patch, fine_transition_cells) and the hollow core on the GPU: the sheet the engine
creates against the numpy restatement of InitParticles (tests/plasma_init_reference.py), the limits in which the feature must
equal a plain deck, the non-uniform sheet through every particle path, and the refusals.

Tolerances of the sheet comparison: positions to 1e-14 of the box width, weights to a relative 1e-14 -- a handful of
roundings and the GPU's fused multiply-adds, far below the lattice spacing; counts, momenta and psi exactly."""
import numpy as np
import pytest

from hipace_amd import decks
from tests import plasma_init_reference as R
from tests.util import NCOMP, rel_err, smooth_slab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def disc(radius):
    return decks.fine_patch_disc(radius)


def cell_mask(deck, f):
    nx, ny = deck["nx"], deck["ny"]
    dx, dy = (deck["hi"][0] - deck["lo"][0]) / nx, (deck["hi"][1] - deck["lo"][1]) / ny
    x = deck["lo"][0] + (np.arange(nx) + 0.5) * dx
    y = deck["lo"][1] + (np.arange(ny) + 0.5) * dy
    return np.broadcast_to(np.asarray(f(x[None, :], y[:, None])), (ny, nx)) > 0


def short_deck(base=None, nz=20, **kw):
    """the blowout deck around the driver's centre: nz slices of the reference's thickness"""
    d = base if base is not None else decks.blowout_wake()
    h = 0.06 * nz
    d.update(nz=nz, n_steps=1, lo=(d["lo"][0], d["lo"][1], -h), hi=(d["hi"][0], d["hi"][1], h), beam_zmin=-h + 0.01, beam_zmax=h - 0.01)
    d.update(decks.PLASMA_INIT_DEFAULT)
    d.update(kw)
    return d


def table_value(x, f, v):
    """common.h: table_value, operation by operation"""
    x, f, v = np.asarray(x, float), np.asarray(f, float), np.asarray(v, float)
    k = np.clip(np.searchsorted(x, v, side="left"), 1, len(x) - 1)
    t = (v - x[k - 1]) / (x[k] - x[k - 1])
    out = f[k - 1] + t * (f[k] - f[k - 1])
    return np.where(v <= x[0], f[0], np.where(v >= x[-1], f[-1], out))


def restated(deck, species, mask, T, density_func=None):
    si = bool(deck.get("si_units", 0))
    ppc = deck["plasma_ppc"] if species == "plasma" else deck["ion_ppc"]
    fine = deck["plasma_fine_ppc"] if species == "plasma" else deck["ion_fine_ppc"]
    dens = deck["plasma_density"] if species == "plasma" else deck["ion_density"]
    radius = deck["plasma_radius"] if deck["plasma_radius"] > 0.0 else np.inf
    use = mask is not None and any(fine)
    return R.init_particles(deck["nx"], deck["ny"], deck["lo"], deck["hi"], deck["nz"], tuple(ppc), tuple(fine) if use else None,
                            mask if use else None, T, density=dens, radius=radius,
                            hollow_core_radius=deck.get("plasma_hollow_core_radius", 0.0), normalized=not si, density_func=density_func)


def assert_sheet(real, valid, ref, deck, ppc, fine):
    """the engine's sheet (any order, invalid slots included) against the restatement, as sets sorted by (y, x)"""
    width = deck["hi"][0] - deck["lo"][0]
    keep = valid != 0
    nslots = ppc[0] * ppc[1] * deck["nx"] * deck["ny"] + (fine[0] * fine[1] - ppc[0] * ppc[1]) * int((ref["L"] > 0).sum())
    assert real.shape[1] == nslots
    assert int(keep.sum()) == ref["x"].size
    gx, gy, gw = R.sort_yx(real[0][keep], real[1][keep], real[2][keep], width=width)
    rx, ry, rw = R.sort_yx(ref["x"], ref["y"], ref["w"], width=width)
    ex, ey, ew = np.abs(gx - rx).max() / width, np.abs(gy - ry).max() / width, np.abs(gw / rw - 1.0).max()
    print(f"sheet: {keep.sum()} of {nslots} slots valid, dx {ex:.2e} dy {ey:.2e} of the width, dw {ew:.2e} relative")
    assert ex <= 1e-14 and ey <= 1e-14 and ew <= 1e-14
    assert np.all(real[3][keep] == 0.0) and np.all(real[4][keep] == 0.0) and np.all(real[5][keep] == 1.0)      # ux, uy, psi
    assert np.array_equal(real[6][keep], real[0][keep]) and np.array_equal(real[7][keep], real[1][keep])        # x_prev, y_prev
    assert np.all(real[8][keep] == 0.0) and np.all(real[9][keep] == 0.0) and np.all(real[10][keep] == 1.0)      # half-step copies
    assert np.all(real[2][~keep] == 0.0) and np.all(real[10][~keep] == 0.0)                                       # invalid slots


# ---- 1. the sheet against the restatement -------------------------------------------------------------------------------------

SHEET_CASES = {
    # name: (ppc, fine, T, tile_size, deck changes)
    "1x1_4x4_T0": ((1, 1), (4, 4), 0, 16, {}),
    "1x1_4x4_T2": ((1, 1), (4, 4), 2, 0, {}),
    "1x1_4x4_T5": ((1, 1), (4, 4), 5, 32, {}),
    "2x2_4x4_T2": ((2, 2), (4, 4), 2, 16, {}),
    "1x1_2x4_T5": ((1, 1), (2, 4), 5, 16, {}),
    "1x1_2x4_T0": ((1, 1), (2, 4), 0, 0, {}),
    "SI_1x1_4x4_T2": ((1, 1), (4, 4), 2, 16, "SI"),
    "SI_2x2_4x4_T5": ((2, 2), (4, 4), 5, 0, "SI"),
    "radius5_hollow1": ((1, 1), (4, 4), 2, 16, dict(plasma_radius=5.0, plasma_hollow_core_radius=1.0)),
    "63x63": ((1, 1), (4, 4), 2, 16, dict(nx=63, ny=63)),
}


@pytest.mark.parametrize("case", sorted(SHEET_CASES))
def test_sheet_matches_the_restatement(api, case):
    ppc, fine, T, ts, changes = SHEET_CASES[case]
    if changes == "SI":
        deck = short_deck(decks.blowout_wake_SI(), nz=4)
        kp_inv = deck["hi"][0] / 8.0
        deck.update(lo=(deck["lo"][0], deck["lo"][1], -0.24 * kp_inv), hi=(deck["hi"][0], deck["hi"][1], 0.24 * kp_inv),
                    beam_zmin=-0.2 * kp_inv, beam_zmax=0.2 * kp_inv)
        patch = disc(2.0 * kp_inv)
    else:
        deck = short_deck(nz=4, **changes)
        patch = disc(2.0)
    deck.update(plasma_ppc=ppc, plasma_fine_ppc=fine)
    eng = api.SliceEngine(deck, tile_size=ts, fine_patch=patch, fine_transition_cells=T)
    eng.begin_step()
    real, valid = eng.particles()
    ref = restated(deck, "plasma", cell_mask(deck, patch), T)
    assert set(np.unique(ref["L"])) == set(range(T + 2))
    assert eng.nparticles == real.shape[1]
    assert_sheet(real, valid, ref, deck, ppc, fine)
    if "radius" in case:
        r = np.hypot(real[0], real[1])[valid != 0]
        assert r.min() >= 1.0 and r.max() <= 5.0 and (valid == 0).sum() > 0


def test_sheet_radius_crop_ignores_the_mask_outside_the_box(api):
    """CPU test 5 on the engine: with a finite radius the map lives on the cropped box.  A mask set everywhere outside the box
    changes nothing; one more fine cell in the box's corner grows its transition inside the box only."""
    T = 3
    deck = short_deck(nz=4, plasma_radius=3.0, plasma_fine_ppc=(4, 4))
    dx = (deck["hi"][0] - deck["lo"][0]) / deck["nx"]
    ilo, ihi, jlo, jhi = R.cell_box(deck["nx"], deck["ny"], deck["lo"], dx, dx, 3.0)
    assert 0 < ilo < ihi < deck["nx"] - 1
    mask = np.ones((deck["ny"], deck["nx"]), bool)
    mask[jlo:jhi + 1, ilo:ihi + 1] = False
    eng = api.SliceEngine(deck, tile_size=16, fine_patch=mask, fine_transition_cells=T)
    eng.begin_step()
    real, valid = eng.particles()
    plain = api.SliceEngine(dict(deck, plasma_fine_ppc=(0, 0)), tile_size=16)
    plain.begin_step()
    preal, pvalid = plain.particles()
    assert np.array_equal(real, preal) and np.array_equal(valid, pvalid)
    assert_sheet(real, valid, restated(deck, "plasma", mask, T), deck, (1, 1), (4, 4))
    mask[jlo, ilo] = True
    eng = api.SliceEngine(deck, tile_size=16, fine_patch=mask, fine_transition_cells=T)
    eng.begin_step()
    ref = restated(deck, "plasma", mask, T)
    assert (ref["L"] > 0).sum() == (T + 1) * (T + 2) // 2            # a quarter of the diamond
    assert_sheet(*eng.particles(), ref, deck, (1, 1), (4, 4))


def test_sheet_of_a_later_step_with_a_time_dependent_profile(api):
    """set_step(3) with n = n0 f_r(r) f_t(c t): the slots stay, the weights scale with f_t"""
    T, patch = 2, disc(2.0)
    deck = short_deck(nz=4, plasma_fine_ppc=(4, 4), plasma_radius=6.0, dt=2.0, beam_umean=(0.0, 0.0, 1.0e6), beam_n_subcycles=1)
    r, fr = np.array([0.0, 1.0, 2.0, 4.0, 6.0]), np.array([1.0, 1.05, 1.2, 1.8, 2.8])
    ct, ft = np.array([0.0, 12.0]), np.array([0.25, 1.0])
    mask = cell_mask(deck, patch)
    sheets = []
    for step in (0, 3):
        eng = api.SliceEngine(deck, tile_size=16, fine_patch=patch, fine_transition_cells=T)
        eng.set_density_profile(r, fr, ct, ft)
        eng.set_step(step)
        eng.begin_step()
        real, valid = eng.particles()
        f_t = float(table_value(ct, ft, 2.0 * step))
        assert f_t == (0.25 if step == 0 else 0.625)
        ref = restated(deck, "plasma", mask, T, density_func=lambda x, y: 1.0 * table_value(r, fr, np.sqrt(x * x + y * y)) * f_t)
        assert_sheet(real, valid, ref, deck, (1, 1), (4, 4))
        sheets.append((real, valid))
    (r0, v0), (r3, v3) = sheets
    assert r0.shape == r3.shape and np.array_equal(v0, v3) and np.array_equal(r0[:2], r3[:2])
    live = v0 != 0
    assert np.abs(r3[2][live] / r0[2][live] - 2.5).max() <= 1e-14


@pytest.mark.parametrize("ionize", [False, True])
def test_ion_sheet_matches_the_restatement(api, ionize):
    """the species "ion" on the same patch with its own fine_ppc; the electrons' capacity follows the ions' count"""
    T, patch = 2, disc(2.0)
    deck = short_deck(nz=4, plasma_fine_ppc=(4, 4), ion_fine_ppc=(2, 2), background_density_SI=1.0e24)
    decks.with_ion_species(deck, "H", 1.0, ppc=(1, 1), initial_level=0 if ionize else 1)
    eng = api.SliceEngine(deck, tile_size=16, fine_patch=patch, fine_transition_cells=T)
    eng.begin_step()
    mask = cell_mask(deck, patch)
    assert_sheet(*eng.particles(), restated(deck, "plasma", mask, T), deck, (1, 1), (4, 4))
    real, valid, lev, key = eng.ions()
    ref = restated(deck, "ion", mask, T)
    assert_sheet(real, valid, ref, deck, (1, 1), (2, 2))
    assert np.all(lev == (0 if ionize else 1))
    assert sorted(key) == list(range(real.shape[1]))                 # slot index + 1 in the id bits
    # the key is the slot: slot k of i_part 0 is cell k
    dx = (deck["hi"][0] - deck["lo"][0]) / deck["nx"]
    first = key < deck["nx"] * deck["ny"]
    cell = np.floor((real[1][first] - deck["lo"][1]) / dx).astype(int) * deck["nx"] + np.floor((real[0][first] - deck["lo"][0]) / dx).astype(int)
    assert np.array_equal(cell, key[first])


# ---- 2., 3. all-true and all-false masks against plain decks --------------------------------------------------------------------

def _lockstep(api, oracle, fine_deck, mask, plain_deck, tile_size):
    """the fine-patch engine, the plain engine and the oracle on the plain deck: bit-equal sheets after begin_step, the fine-patch
    engine's slab against the oracle's slice by slice (the tolerances of test_engine_slice_by_slice_vs_oracle), checksums of
    the two engines to a relative 1e-9 after the step"""
    fe = api.SliceEngine(fine_deck, tile_size=tile_size, sort_period=5, fine_patch=mask, fine_transition_cells=2)
    pe = api.SliceEngine(plain_deck, tile_size=tile_size, sort_period=5)
    oe = oracle.Engine(plain_deck)
    for e in (fe, pe):
        e.set_diagnostics(True)
        e.begin_step()
    oe.begin_step()
    freal, fvalid = fe.particles()
    preal, pvalid = pe.particles()
    assert freal.shape == preal.shape and np.array_equal(fvalid, pvalid)
    assert np.array_equal(freal, preal)                                     # bit-equal
    from hipace_amd._lib import COMPS
    for isl in range(fine_deck["nz"] - 1, -1, -1):
        for e in (fe, pe, oe):
            e.solve_slice(isl)
        if isl % 6 == 0:
            gs, os_ = fe.slab(), oe.slab()
            for c in range(fe.ncomp):
                assert rel_err(gs[c], os_[c]) < 1e-9, (isl, COMPS[c], rel_err(gs[c], os_[c]))
    fc, pc = fe.checksums(), pe.checksums()
    assert any(v != 0.0 for v in pc.values())
    for k, v in pc.items():
        if v != 0.0:
            assert abs(fc[k] - v) <= 1e-9 * abs(v), (k, fc[k], v)
    greal, gvalid = fe.particles()
    oreal, ovalid = oe.particles()
    gk = np.lexsort((np.round(greal[0], 7), np.round(greal[1], 7)))
    ok = np.lexsort((np.round(oreal[0], 7), np.round(oreal[1], 7)))
    assert np.array_equal(gvalid[gk], ovalid[ok])
    for k in range(11):
        assert rel_err(greal[k][gk], oreal[k][ok]) < 1e-9, k


@pytest.mark.parametrize("tile_size", [0, 16])
def test_all_true_mask_is_the_uniform_fine_deck(api, oracle, tile_size):
    fine = short_deck(plasma_ppc=(1, 1), plasma_fine_ppc=(2, 2))
    plain = short_deck(plasma_ppc=(2, 2))
    _lockstep(api, oracle, fine, np.ones((64, 64), bool), plain, tile_size)


@pytest.mark.parametrize("tile_size", [0, 16])
def test_all_false_mask_is_the_deck_without_a_patch(api, oracle, tile_size):
    fine = short_deck(plasma_ppc=(1, 1), plasma_fine_ppc=(4, 4))
    plain = short_deck(plasma_ppc=(1, 1))
    _lockstep(api, oracle, fine, np.zeros((64, 64), bool), plain, tile_size)


# ---- 4. hollow core against the oracle ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile_size", [0, 16])
def test_hollow_core_matches_the_oracle_with_a_stepped_profile(api, oracle, tile_size):
    r_h = 1.3
    deck = short_deck(nz=10, plasma_hollow_core_radius=r_h)
    dx = (deck["hi"][0] - deck["lo"][0]) / deck["nx"]
    c = deck["lo"][0] + (np.arange(deck["nx"]) + 0.5) * dx
    radii = np.unique(np.hypot(c[None, :], c[:, None]))
    assert np.abs(radii - r_h).min() > 1e-6
    ra, rb = radii[radii < r_h].max(), radii[radii > r_h].min()
    ge = api.SliceEngine(deck, tile_size=tile_size, sort_period=5)
    oe = oracle.Engine(deck)                               # (the oracle does not know the key: the profile stands for it)
    oe.set_density_profile(np.array([ra, rb]), np.array([0.0, 1.0]), np.array([]), np.array([]))
    ge.begin_step()
    oe.begin_step()
    from hipace_amd._lib import COMPS
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        gs, os_ = ge.slab(), oe.slab()
        for comp in range(ge.ncomp):
            assert rel_err(gs[comp], os_[comp]) < 1e-9, (isl, COMPS[comp], rel_err(gs[comp], os_[comp]))
    gr, gv = ge.particles()
    orl, ov = oe.particles()
    keep = gv != 0
    assert keep.sum() == orl.shape[1] == int(ov.sum()) == int((np.hypot(c[None, :], c[:, None]) > r_h).sum()) < gv.size
    kg = np.lexsort((np.round(gr[7][keep], 9), np.round(gr[6][keep], 9)))
    ko = np.lexsort((np.round(orl[7], 9), np.round(orl[6], 9)))
    for q in range(11):
        assert rel_err(gr[q][keep][kg], orl[q][ko]) < 1e-9, q


# ---- 5. the non-uniform sheet through every particle path ------------------------------------------------------------------------

def _variant(name):
    if name == "laser":
        d = short_deck(decks.laser_blowout_wake())
        d.update(nx=64, ny=64, lo=(-16.0, -16.0, d["lo"][2]), hi=(16.0, 16.0, d["hi"][2]))
        patch = disc(4.0)
    else:
        d, patch = short_deck(), disc(2.0)
    d.update(plasma_ppc=(1, 1), plasma_fine_ppc=(4, 4))
    if name == "predictor_corrector":
        d = decks.predictor_corrector(d)
    elif name in ("ion", "ion_ionizing"):
        d.update(ion_fine_ppc=(2, 2), background_density_SI=1.0e24)
        decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=0 if name == "ion_ionizing" else 1)
        if name == "ion":
            d.update(plasma_no_neutralize=1)
    elif name == "moving_beam":
        d.update(dt=0.9)
    elif name == "collisions":
        d.update(background_density_SI=1.0e24, collisions=[(0, 0, -1.0, 0)])
    return d, patch


@pytest.mark.parametrize("name", ["explicit", "predictor_corrector", "ion", "ion_ionizing", "laser", "moving_beam", "collisions"])
def test_non_uniform_sheet_any_tiling(api, name):
    """the disc patch (1x1 -> 4x4, T = 2: 16 particles per cell from slice 0 on, the rank cap of the tile sort) for one whole
    step: tile sizes 16 (re-sorted every slice) and 32 (every 7th at the latest) against the per-particle kernels"""
    deck, patch = _variant(name)
    out = {}
    for ts, period in ((0, 1), (16, 1), (32, 7)):
        eng = api.SliceEngine(deck, tile_size=ts, sort_period=period, fine_patch=patch, fine_transition_cells=2)
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
    assert out[0][1] == 0 and out[0][2] == 0                 # no tiles: nothing can leave one, nothing is sorted
    if name == "ion_ionizing":
        assert out[0][3][0] > 0
    if name == "ion":
        assert out[0][3][0] == 0


@pytest.mark.parametrize("ts", [16, 32])
def test_fused_schedule_on_the_patch_sheet(api, ts):
    """hps_engine_set_fusion takes the non-uniform sheet: the bar of test_fused_push_and_deposit_schedule, fused against the
    two-kernel schedule after every few slices, with the patch set before and after the switch"""
    deck, patch = _variant("explicit")
    a = api.SliceEngine(deck, tile_size=ts, sort_period=7, fine_patch=patch, fine_transition_cells=2)
    b = api.SliceEngine(deck, tile_size=ts, sort_period=7, fine_patch=patch if ts == 16 else None, fine_transition_cells=2)
    b.set_fusion(True)
    if ts == 32:
        b.set_fine_patch(patch, 2)
    for e in (a, b):
        e.set_diagnostics(True)
        e.begin_step()
    names = a.comp_names()
    ahead = {"jx", "jy", "chi", "rhomjz", "rho", "jx_beam", "jy_beam", "jz_beam", "N_jx_beam", "N_jy_beam", "P_jx_beam", "P_jy_beam"}
    for k in range(deck["nz"] - 1, -1, -1):
        a.solve_slice(k)
        b.solve_slice(k)
        if k % 6 == 0:
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
    ca, cb = a.checksums(), b.checksums()
    assert sum(v != 0.0 for v in ca.values()) >= 8
    for nm, v in ca.items():
        assert abs(cb[nm] - v) <= 1e-10 * max(abs(v), 1e-300), (nm, cb[nm], v)


# ---- 6. the operators on the non-uniform sheet against the oracle ----------------------------------------------------------------

@pytest.mark.parametrize("ts", [16, 32])
def test_tiled_operators_on_the_patch_sheet_vs_oracle(api, oracle, ts):
    deck, patch = _variant("explicit")
    eng = api.SliceEngine(deck, tile_size=0, fine_patch=patch, fine_transition_cells=2)
    eng.begin_step()
    real, valid = eng.particles()
    n, order, g = deck["nx"], deck["order"], (deck["order"] + 1) // 2 + 1
    lo, hi = deck["lo"][:2], deck["hi"][:2]
    ion = np.zeros(real.shape[1], dtype=np.int32)
    # a cold sheet is a poor test of the push and of the current: give it a seeded thermal spread
    rng = np.random.default_rng(ts)
    real = real.copy()
    real[3], real[4] = 0.3 * rng.standard_normal(real.shape[1]), 0.3 * rng.standard_normal(real.shape[1])
    real[5] = np.sqrt(1.0 + real[3] ** 2 + real[4] ** 2)
    real[8], real[9], real[10] = real[3], real[4], real[5]
    geom = api.Geometry(n, n, lo, hi, 0.3)
    ogeom = oracle.make_geom(n, n, lo, hi, dz=0.3, bc=1)
    til = api.Tiling(n, n, ts, real.shape[1])
    sheet = til.reorder(api.PlasmaSheet(real, valid, ion), geom)
    sreal, svalid = sheet.numpy()
    off, _ = til.offsets_and_perm(real.shape[1])
    counts = np.diff(off[:til.info()[0] + 1])
    # the patch's centre is a tile corner: the tiles around it hold a quarter of the disc at 16 per cell, the others 1 per cell
    assert counts.sum() == int(valid.sum()) and counts.max() >= ts * ts + 15 * 50 and (ts == 32 or counts.min() == ts * ts)
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


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(api):
    def fails(fn, needle):
        with pytest.raises(RuntimeError) as ei:
            fn()
        assert needle in str(ei.value), str(ei.value)

    base = short_deck(nz=4)
    mask = np.ones((64, 64), bool)
    # fine_ppc not divisible by ppc, component by component
    fails(lambda: api.SliceEngine(dict(base, plasma_ppc=(2, 2), plasma_fine_ppc=(4, 3)), fine_patch=mask), "divisible by ppc")
    fails(lambda: api.SliceEngine(dict(base, plasma_ppc=(2, 1), plasma_fine_ppc=(3, 4)), fine_patch=mask), "divisible by ppc")
    fails(lambda: api.SliceEngine(dict(base, plasma_fine_ppc=(4, 0)), fine_patch=mask), "divisible by ppc")
    fails(lambda: api.SliceEngine(dict(base, ion_fine_ppc=(2, 2)), fine_patch=mask), "ion species")
    ion = decks.with_ion_species(dict(base, background_density_SI=1.0e24), "H", 1.0, ppc=(2, 2))
    fails(lambda: api.SliceEngine(dict(ion, ion_fine_ppc=(3, 2)), fine_patch=mask), "divisible by its ppc")
    # exactly one of fine_ppc and the patch: at the first begin_step
    eng = api.SliceEngine(dict(base, plasma_fine_ppc=(4, 4)))
    fails(eng.begin_step, "both fine_ppc")
    eng = api.SliceEngine(base, fine_patch=mask)
    fails(eng.begin_step, "both fine_ppc")
    # transition cells, hollow core
    fails(lambda: api.SliceEngine(dict(base, plasma_fine_ppc=(4, 4)), fine_patch=mask, fine_transition_cells=-1), "must not be negative")
    fails(lambda: api.SliceEngine(dict(base, plasma_radius=3.0, plasma_hollow_core_radius=3.0)), "smaller than the plasma radius")
    fails(lambda: api.SliceEngine(dict(base, plasma_radius=3.0, plasma_hollow_core_radius=4.0)), "smaller than the plasma radius")
    fails(lambda: api.SliceEngine(dict(base, plasma_hollow_core_radius=-1.0)), "must not be negative")
    with pytest.raises(ValueError):
        api.SliceEngine(dict(base, plasma_fine_ppc=(4, 4)), fine_patch=np.ones((64, 63), bool))
    # after the first begin_step
    eng = api.SliceEngine(dict(base, plasma_fine_ppc=(4, 4)), fine_patch=mask)
    eng.begin_step()
    fails(lambda: eng.set_fine_patch(mask, 2), "before the first hps_engine_begin_step")


@pytest.mark.parametrize("first", ["tiling", "patch"])
def test_set_tiling_before_or_after_the_patch(api, first):
    deck, patch = _variant("explicit")
    deck.update(nz=4)
    eng = api.SliceEngine(deck)
    if first == "tiling":
        eng.set_tiling(32, 3)
        eng.set_fine_patch(patch, 2)
    else:
        eng.set_fine_patch(patch, 2)
        eng.set_tiling(32, 3)
    eng.begin_step()
    assert_sheet(*eng.particles(), restated(deck, "plasma", cell_mask(deck, patch), 2), deck, (1, 1), (4, 4))
    eng.solve_slice(deck["nz"] - 1)
    assert eng.sorts() > 0
