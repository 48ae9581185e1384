"""Parsed plasma densities on the GPU (hps_engine_set_density_expr): the sheets the program variants of the init
kernels make, slot for slot against the restatement of InitParticles with the host evaluation of the program
(tests/density_expr_reference.py); the two species; the deepest stack; min_density; the limits in which a program must equal
the deck or the tables; the laser's initial chi; the density table; the reference's own lwfa deck; the refusals.

Arithmetic programs (+ - * /, integer powers, comparisons, if) are compared bit for bit: the GPU, hps_expr_eval_host and numpy
round alike, and the weight is one multiplication on top."""
import json
import os

import numpy as np
import pytest

from hipace_amd import decks, expr
from tests import density_expr_reference as D
from tests import laser_grid_reference as LG

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROG = "1 + 0.3*x*y/16 + 0.05*z*x + if(x > 4 and y < -3, -5, 0)"      # non-separable; removes a corner


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def box_deck(nx=24, ny=20, **kw):
    """24 x 20 cells on (-6, 6) x (-5, 5), two particles per cell in x: 960 slots, three full blocks and a partial one"""
    d = decks.blowout_wake()
    d.update(nx=nx, ny=ny, nz=4, n_steps=3, lo=(-6.0, -5.0, -0.24), hi=(6.0, 5.0, 0.24), beam_zmin=-0.23, beam_zmax=0.23,
             plasma_ppc=(2, 1), dt=2.0, beam_umean=(0.0, 0.0, 1.0e6), beam_n_subcycles=1)
    d.update(decks.PLASMA_INIT_DEFAULT)
    d.update(decks.PLASMA_THERMAL_DEFAULT)
    d.update(kw)
    return d


def sheet_at_step(api, deck, step, tile_size, setup, **engine_kw):
    eng = api.SliceEngine(deck, tile_size=tile_size, **engine_kw)
    setup(eng)
    eng.set_step(step)
    eng.begin_step()
    return eng


# ---- 5. the sheet, slot for slot ---------------------------------------------------------------------------------------------

def _mask_6x6():
    m = np.zeros((20, 24), dtype=bool)
    m[7:13, 9:15] = True
    return m


INIT_PATHS = {
    # name: (deck changes, fine-patch mask, T)
    "plain": (dict(), None, 5),
    "fine_hollow": (dict(plasma_fine_ppc=(4, 2), plasma_hollow_core_radius=1.0), _mask_6x6(), 2),
    "warm": (dict(plasma_u_std=(0.01, 0.01, 0.01), plasma_seed=3), None, 5),
    "warm_sym_prevent": (dict(nx=21, ny=19, plasma_u_std=(0.01, 0.01, 0.01), plasma_seed=3, plasmas_do_symmetrize=1,
                              plasmas_prevent_centered_particle=1), None, 5),
}


@pytest.mark.parametrize("tile_size", [0, 16])
@pytest.mark.parametrize("path", sorted(INIT_PATHS))
def test_sheet_slot_for_slot(api, path, tile_size):
    changes, mask, T = INIT_PATHS[path]
    deck = box_deck(**changes)
    kw = dict(fine_patch=mask, fine_transition_cells=T) if mask is not None else {}
    width = deck["hi"][0] - deck["lo"][0]
    for step in range(3):
        z = deck["dt"] * step
        eng = sheet_at_step(api, deck, step, 0, lambda e: e.set_density_expr("plasma", PROG), **kw)
        real, valid = eng.particles()
        lat = D.lattice(deck, "plasma", mask, T, step=step)
        ref = D.expected(lat, PROG, z)
        kept, dead = D.assert_sheet(real, valid, ref, PROG, z, width)
        if tile_size:      # the tile sort permutes the sheet: the same particles, sorted by (y, x)
            tiled = sheet_at_step(api, deck, step, tile_size, lambda e: e.set_density_expr("plasma", PROG), **kw)
            D.assert_same_particles(*tiled.particles(), real, valid)
        removed_by_program = int((~ref["kept"]).sum())
        print(f"{path} tile {tile_size} step {step}: {kept} kept, {dead} invalid slots, {removed_by_program} removed by the program")
        assert kept > 0 and removed_by_program > 0 and kept + dead == real.shape[1]
        assert np.all(real[2][valid != 0] > 0.0)


# ---- 6. two species, two programs ---------------------------------------------------------------------------------------------

def ion_deck(**kw):
    d = box_deck(background_density_SI=1.0e24, **kw)
    decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=1)
    return d


def test_two_species_two_programs(api):
    deck = ion_deck()
    width = deck["hi"][0] - deck["lo"][0]
    pe, pi = "1 + 0.1*x", "2 - 0.1*y"
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_density_expr("plasma", pe)
    eng.set_density_expr("ion", pi)
    eng.begin_step()
    real, valid = eng.particles()
    kept, dead = D.assert_sheet(real, valid, D.expected(D.lattice(deck, "plasma"), pe, 0.0), pe, 0.0, width)
    assert kept == 960 and dead == 0
    ireal, ivalid, lev, key = eng.ions()
    o = np.argsort(key)                                  # the ions' sheet is tile-sorted; the key is the slot
    assert np.array_equal(key[o], np.arange(480))
    kept, dead = D.assert_sheet(ireal[:, o], ivalid[o], D.expected(D.lattice(deck, "ion"), pi, 0.0), pi, 0.0, width)
    assert kept == 480 and dead == 0 and np.all(lev == 1)
    assert not np.array_equal(real[2][:480], ireal[2][o])
    # a program on the ions alone: the plasma stays on the tables, bit for bit the sheet of an engine without any program
    prof = (np.array([0.0, 2.0, 7.0]), np.array([1.0, 1.1, 2.0]), np.array([0.0, 4.0]), np.array([0.5, 1.0]))
    only_ion = api.SliceEngine(deck, tile_size=0)
    only_ion.set_density_profile(*prof)
    only_ion.set_density_expr(1, pi)
    only_ion.begin_step()
    none = api.SliceEngine(deck, tile_size=0)
    none.set_density_profile(*prof)
    none.begin_step()
    (ra, va), (rb, vb) = only_ion.particles(), none.particles()
    assert np.array_equal(ra.view(np.uint64), rb.view(np.uint64)) and np.array_equal(va, vb)
    jreal, jvalid, _, jkey = only_ion.ions()
    o2 = np.argsort(jkey)
    assert np.array_equal(jreal[:, o2].view(np.uint64), ireal[:, o].view(np.uint64))
    treal, _, _, tkey = none.ions()
    assert not np.array_equal(treal[2][np.argsort(tkey)], jreal[2][o2])


# ---- 7. the deepest program -----------------------------------------------------------------------------------------------------

def deepest_program():
    """stack depth 16 and 256 instructions, arithmetic only: sixteen operands nested to the right (31 instructions), a unary
    minus, and 112 additions of a constant, unfolded"""
    inner = "x+(y+(z+(0.5+(x+(y+(1.25+(x+(y+(0.75+(x+(y+(2+(x+(y+3"
    text = "-(" + inner + ")" * 14 + ")"
    text += " + 0.5 - 0.25 + 0.125 - 0.375" * 28
    p = expr.compile_expr(text, ("x", "y", "z"), fold=False)
    assert p.depth == expr.MAX_DEPTH == 16 and len(p.ins) == expr.MAX_INS == 256, (p.depth, len(p.ins))
    return p


def test_deepest_program(api):
    deck = box_deck()
    width = deck["hi"][0] - deck["lo"][0]
    lat = D.lattice(deck, "plasma")
    deep, shallow = deepest_program(), expr.compile_expr("x + 7", ("x", "y", "z"))
    assert shallow.depth == 2
    for prog, lds in ((deep, 15 * 256 * 8), (shallow, 1 * 256 * 8)):
        assert (prog.depth - 1) * 256 * 8 == lds <= 30720
        eng = sheet_at_step(api, deck, 1, 0, lambda e: e.set_density_expr(0, prog, min_density=-1.0e3))
        real, valid = eng.particles()
        ref = D.expected(lat, prog, 2.0, min_density=-1.0e3)
        kept, dead = D.assert_sheet(real, valid, ref, prog, 2.0, width)
        assert kept == 960 and dead == 0 and np.unique(real[2]).size >= 48      # (the lattice has 48 distinct x)


# ---- 8. min_density -----------------------------------------------------------------------------------------------------------

def test_min_density(api):
    deck = box_deck()
    width = deck["hi"][0] - deck["lo"][0]
    lat = D.lattice(deck, "plasma")
    prog = "1 + 0.2*x"
    eng = sheet_at_step(api, deck, 0, 0, lambda e: e.set_density_expr(0, prog, min_density=0.5))
    real, valid = eng.particles()
    ref = D.expected(lat, prog, 0.0, min_density=0.5)
    kept, dead = D.assert_sheet(real, valid, ref, prog, 0.0, width)
    value = 1.0 + 0.2 * lat["x"]
    assert kept == int((value > 0.5).sum()) and 0 < kept < 960 and dead == 960 - kept
    assert real[0][valid != 0].min() > -2.5 and real[2][valid != 0].min() > 0.5 * 0.5      # value > 0.5, scale_fac = 1/2
    # the reference creates whatever lies above min_density, negative weights included
    prog = "0.2*x"
    eng = sheet_at_step(api, deck, 0, 0, lambda e: e.set_density_expr(0, prog, min_density=-10.0))
    real, valid = eng.particles()
    kept, dead = D.assert_sheet(real, valid, D.expected(lat, prog, 0.0, min_density=-10.0), prog, 0.0, width)
    assert kept == 960 and dead == 0 and (real[2] < 0.0).sum() == 480


# ---- 9. the constant program is the deck ---------------------------------------------------------------------------------------

def test_constant_program_is_the_deck(api):
    deck = decks.blowout_wake()
    deck.update(nx=32, ny=32, nz=20, n_steps=1, lo=(-8.0, -8.0, -1.2), hi=(8.0, 8.0, 1.2), beam_zmin=-1.1, beam_zmax=1.1)
    a, b = api.SliceEngine(deck, tile_size=16), api.SliceEngine(deck, tile_size=16)
    a.set_density_expr("plasma", deck["plasma_density"])
    a.begin_step()
    b.begin_step()
    (ra, va), (rb, vb) = a.particles(), b.particles()
    assert np.array_equal(ra.view(np.uint64), rb.view(np.uint64)) and np.array_equal(va, vb) and va.all()
    for k in range(deck["nz"] - 1, deck["nz"] - 4, -1):
        a.solve_slice(k)
        b.solve_slice(k)
    sa, sb = a.slab(), b.slab()
    for c, name in enumerate(a.comp_names()):
        assert np.abs(sa[c] - sb[c]).max() <= 1e-9 * max(np.abs(sb[c]).max(), 1e-300), name
    assert np.abs(sb).max() > 0.0


# ---- 10. against the tables and the oracle -------------------------------------------------------------------------------------

def table_as_program(r, fr, ramp):
    """the piecewise-linear f_r(sqrt(x^2 + y^2)) of common.h: table_value as nested ifs over the knots, times the ramp"""
    R = "sqrt(x^2 + y^2)"
    text = repr(float(fr[-1]))
    for k in range(len(r) - 1, 0, -1):
        seg = f"({fr[k - 1]!r} + ({R} - {r[k - 1]!r})/{r[k] - r[k - 1]!r}*{fr[k] - fr[k - 1]!r})"
        text = f"if({R} < {r[k]!r}, {seg}, {text})"
    return f"{text} * ({ramp})"


@pytest.mark.parametrize("tile_size", [0, 16])
def test_program_of_the_tables_matches_the_oracle(api, oracle, tile_size):
    """the deck and the checks of tests/test_gpu_parity.py::test_plasma_density_profile_matches_oracle, the GPU engine on the
    program, the oracle on the tables"""
    deck = decks.blowout_wake()
    deck.update(nz=20, lo=(-8.0, -8.0, -1.2), hi=(8.0, 8.0, 1.2), beam_zmin=-1.1, beam_zmax=1.1, n_steps=3, dt=2.0, plasma_ppc=(2, 2),
                beam_umean=(0.0, 0.0, 1.0e6), beam_n_subcycles=1)
    r = [0.0, 1.0, 2.0, 4.0, 6.0, 6.01]
    fr = [1.0, 1.05, 1.2, 1.8, 2.8, 0.0]
    ct, ft = np.array([0.0, 4.0]), np.array([0.25, 1.0])
    prog = expr.compile_expr(table_as_program(r, fr, "0.25 + 0.1875*z"), ("x", "y", "z"))
    ge = api.SliceEngine(deck, tile_size=tile_size)
    ge.set_density_expr("plasma", prog)
    oe = oracle.Engine(deck)
    oe.set_density_profile(np.array(r), np.array(fr), ct, ft)
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
        for q in range(11):
            assert np.abs(gr[q][keep][kg] - orl[q][ko]).max() <= 1e-9 * max(np.abs(orl[q]).max(), 1e-300), (step, q)


# ---- 11. the laser's initial chi ------------------------------------------------------------------------------------------------

def test_laser_initial_chi(api):
    """SetInitialChi with programs: a laser grid of 48 x 40 cells on twice the 24 x 20 field box.  The laser cells off the
    field box shrunk by the guard width carry chi_initial as it is (k_laser_interp_chi copies it), so there laser_chi()
    after the first slice of a step is sum_s prog_s(x, y, c t) q_s^2 mu0 / m_s inside the radius and 0 outside it, to the
    5e-15 of DESIGN 8j; without min_density (the plasma's sheet loses x <= -1 to it, chi does not)."""
    d = decks.laser_blowout_wake()
    d.update(nx=24, ny=20, nz=4, lo=(-6.0, -5.0, -0.6), hi=(6.0, 5.0, 0.6), laser_a0=0.5, laser_lambda0=0.4, dt=5.0, n_steps=2,
             laser_solver=1, plasma_radius=5.0, background_density_SI=1.0e24,
             laser_n_cell=(48, 40), laser_patch_lo=(-12.0, -10.0, -0.6), laser_patch_hi=(12.0, 10.0, 0.6), laser_interp_order=1)
    decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=1)
    pe, pi = "1 + 0.1*x", "2 - 0.1*y"
    nxl, nyl, zlo, zhi, lo3, hi3, dxl, dyl, xoffl, yoffl = decks.laser_geometry(d)
    lg = (dxl, dyl, xoffl, yoffl)
    assert (nxl, nyl) == (48, 40)
    eng = api.SliceEngine(d, tile_size=0)
    eng.set_density_expr("plasma", pe, min_density=0.9)
    eng.set_density_expr("ion", pi)
    x, y, _ = eng.laser_cell_centres()
    X, Y = np.meshgrid(x, y)
    g, names = eng.ng, eng.comp_names()
    dx, dy = 0.5, 0.5
    xoff, yoff = LG.pos_offset(-6.0, 6.0, dx, 0, 23), LG.pos_offset(-5.0, 5.0, dy, 0, 19)
    for step in range(2):
        eng.begin_step()
        eng.solve_slice(d["nz"] - 1)
        z = d["dt"] * step
        want = (D.host_value(pe, X, Y, z) * (d["plasma_charge"] ** 2 / d["plasma_mass"])
                + D.host_value(pi, X, Y, z) * (d["ion_charge"] ** 2 / d["ion_mass"] * d["ion_init_level"] ** 2))
        want = np.where(X * X + Y * Y > 25.0, 0.0, want)
        _, inside = LG.interp_chi(eng.slab()[names.index("chi")], want, lg, 24, 20, g, dx, dy, xoff, yoff, g, 1)
        off = ~inside
        got = eng.laser_chi()
        assert (off & (want != 0.0)).sum() >= 8 and (off & (want == 0.0)).sum() > 100      # off the box: inside and beyond the radius
        assert (off & (want != 0.0) & (X < -1.0)).any()                                    # ... and where the sheet has no plasma
        err = np.abs(got[off] - want[off]).max() / np.abs(want[off]).max()
        print(f"step {step}: initial chi off the field box to {err:.2e}")
        assert err <= 5e-15 and np.all(got[off & (want == 0.0)] == 0.0)
        for k in range(d["nz"] - 2, -1, -1):
            eng.solve_slice(k)


# ---- 12. the density table on the engine ---------------------------------------------------------------------------------------

def test_density_table_on_the_engine(api):
    deck = box_deck(dt=1.5)
    width = deck["hi"][0] - deck["lo"][0]
    lat = D.lattice(deck, "plasma")
    table = [(1.0, "1"), (3.0, "2 + 0.1*x"), (5.0, "3")]
    in_force = []
    for step in range(5):
        z = 1.5 * step
        eng = sheet_at_step(api, deck, step, 0, lambda e: e.set_density_expr("plasma", table))
        real, valid = eng.particles()
        k = min(int(np.searchsorted([1.0, 3.0, 5.0], z, side="left")), 2)      # lower_bound, the last entry beyond the table
        in_force.append(k)
        kept, dead = D.assert_sheet(real, valid, D.expected(lat, table[k][1], z), table[k][1], z, width)
        assert kept == 960 and dead == 0
    assert in_force == [0, 1, 1, 2, 2]
    # hps_engine_set_time: the entry and z follow the time given, not dt * step
    table[1] = (3.0, "2 + 0.1*x + 0.25*z")
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_density_expr("plasma", table)
    eng.set_step(4)
    eng.set_time(2.5, 1.5)
    eng.begin_step()
    real, valid = eng.particles()
    kept, dead = D.assert_sheet(real, valid, D.expected(lat, table[1][1], 2.5), table[1][1], 2.5, width)
    assert kept == 960 and dead == 0 and real[2].min() > 0.5 * (2.625 - 0.6)


# ---- 13. the reference's own deck -----------------------------------------------------------------------------------------------

def test_production_lwfa_parsed_matches_the_reference_checksums(api):
    """tests/test_host_beam_gpu.py::test_production_lwfa_deck_matches_the_reference_checksums with plasma.density(x,y,z) as
    examples/get_started/inputs_lwfa writes it, evaluated on the device: the same file, the same tolerances.  Measured
    (DESIGN 8m): the parsed deck holds the file's ten leading sums to 2.8e-13; the tabulated deck holds them to 3e-13."""
    from tests.test_host_beam_gpu import _xz_diagnostic_sums
    gold = json.load(open(os.path.join(GOLD, "production.SI.2Rank_lwfa.json")))["lev=0"]
    deck = decks.production_lwfa_parsed()
    eng = api.SliceEngine(deck, tile_size=16)
    assert set(eng.density_exprs) == {0} and not hasattr(eng, "density_profile")
    for _ in range(deck["n_steps"] - 1):
        eng.run_step()
    names = [k for k in gold if k != "laserEnvelope"]
    sums = _xz_diagnostic_sums(api, eng, deck, names)
    a = eng.laser_envelope()
    ny = deck["ny"]
    sums["laserEnvelope"] = float(np.abs(0.5 * (a[:, ny // 2 - 1, :] + a[:, ny // 2, :])).sum())
    lead = ("By", "ExmBy", "Ez", "Psi", "Sx", "aabs", "chi", "jx", "laserEnvelope", "rhomjz")
    print("distance to the file:", {k: f"{abs(sums[k] - gold[k]) / gold[k]:.2e}" for k in lead})
    for k in lead:
        assert abs(sums[k] - gold[k]) <= 1e-10 * gold[k], (k, sums[k], gold[k])
    for k in ("Bx", "Bz", "EypBx", "Sy", "jy"):
        assert abs(sums[k] - gold[k]) <= 1e-5 * gold[k], (k, sums[k], gold[k])
    for k in ("jx_beam", "jy_beam", "jz_beam"):
        assert sums[k] == 0.0 == gold[k]


# ---- 14. the refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(api):
    import ctypes as C
    from hipace_amd import _lib
    deck = box_deck()
    eng = api.SliceEngine(deck, tile_size=0)
    with pytest.raises(_lib.HpsError, match="no ion species"):
        eng.set_density_expr("ion", "1")
    with pytest.raises(_lib.HpsError, match="variable index beyond n_vars"):
        eng.set_density_expr(0, expr.Program([("var", 3)], [], ("x", "y", "z", "t")))
    with pytest.raises(_lib.HpsError, match="strictly ascending"):
        eng.set_density_expr(0, [(3.0, "1"), (1.0, "2")])
    one, keep = expr.c_programs([expr.compile_expr("1", ("x", "y", "z"))])
    with pytest.raises(_lib.HpsError, match="n_progs must be >= 1"):
        _lib.check(_lib.lib().hps_engine_set_density_expr(eng._h, 0, 0, one, None, 0.0))
    with pytest.raises(_lib.HpsError, match="null engine"):
        _lib.check(_lib.lib().hps_engine_set_density_expr(None, 0, 1, one, None, 0.0))
    with pytest.raises(ValueError, match="unknown name: 't'"):
        eng.set_density_expr(0, "x + t")
    with pytest.raises(ValueError, match="species must be"):
        eng.set_density_expr("electrons", "1")
    no_plasma = api.SliceEngine(dict(deck, plasma_ppc=(0, 0), plasma_density=0.0), tile_size=0)
    with pytest.raises(_lib.HpsError, match="does not have this species"):
        no_plasma.set_density_expr(0, "1")
    assert not hasattr(eng, "density_exprs")             # every refusal left the engine on the deck's density
    eng.begin_step()
    real, valid = eng.particles()
    assert valid.all() and np.all(real[2] == 0.5)
    with pytest.raises(_lib.HpsError, match="before the first hps_engine_begin_step"):
        eng.set_density_expr(0, "1")
