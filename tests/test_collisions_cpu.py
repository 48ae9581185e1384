"""Binary Coulomb collisions, CPU side: the numpy restatement's own properties, the ABI's presence, the deck."""
import os
import re

import numpy as np
import pytest

from tests import collision_reference as R
from hipace_amd import _lib, decks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Conservation per cell with equal weights: what fp64 rounding of the two Lorentz transforms (into the centre-of-mass frame
# and back) leaves of  sum m u  and  sum m gamma , relative to  sum m |u|  and  sum m gamma  of the cell.  Measured on the
# cells of conservation_cases below: 7.4e-15 (momentum), 5.7e-16 (energy); the bound is ten times the larger one.
CONSERVATION_BOUND = 7.4e-14


def _collide(s, lo, dx, si, **kw):
    q, m = (-R.QE, R.ME) if si else (-1.0, 1.0)
    kw.setdefault("background_density_SI", 0.0 if si else 1.0e24)
    return R.collide(s, s, R.NX, R.NY, lo, dx, dx, dx, q, m, normalized=not si, **kw)


def conservation_cases():
    """(name, sheet, lo, dx, si, kwargs): equal weights, one species, every occupancy, fixed and automatic logarithm"""
    out = []
    for si in (False, True):
        for L in (-1.0, 10.0):
            s, lo, dx = R.thermal_cells(11, si=si, equal_weights=True)
            if si:
                s["w"] *= 1.0e8
            out.append((f"si={si} L={L}", s, lo, dx, si, dict(coulomb_log=L, seed=5)))
    return out


def conservation_error(before, after, m, c, lo, dx):
    a, b = R.cell_sums(before, m, c, R.NX, R.NY, lo, dx), R.cell_sums(after, m, c, R.NX, R.NY, lo, dx)
    ep = max(np.abs(b[k][:3] - a[k][:3]).max() / a[k][4] for k in a)
    ee = max(abs(b[k][3] - a[k][3]) / a[k][3] for k in a)
    return ep, ee


def test_reference_conserves_momentum_and_energy_per_cell():
    worst = [0.0, 0.0]
    for name, s, lo, dx, si, kw in conservation_cases():
        before = R.copy_sheet(s)
        log = _collide(s, lo, dx, si, **kw)
        assert log["pairs"] > 300 and log["rejected"] == [0, 0], name
        ep, ee = conservation_error(before, s, R.ME if si else 1.0, R.C_SI if si else 1.0, lo, dx)
        print(f"{name}: momentum {ep:.3e} energy {ee:.3e}")
        worst = [max(worst[0], ep), max(worst[1], ee)]
        assert ep <= CONSERVATION_BOUND and ee <= CONSERVATION_BOUND, (name, ep, ee)
    print(f"worst: momentum {worst[0]:.3e} energy {worst[1]:.3e}")


def test_permuted_sheet_gives_the_same_result_per_key():
    s, lo, dx = R.thermal_cells(3)
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(s["x"]))
    t = {k: v[perm].copy() for k, v in s.items()}
    _collide(s, lo, dx, False, seed=9)
    _collide(t, lo, dx, False, seed=9)
    a, b = np.argsort(s["key"]), np.argsort(t["key"])
    for k in ("ux", "uy", "psi"):
        assert np.array_equal(s[k][a], t[k][b]), k


def test_odd_counts_pair_with_wrap_around():
    # three particles in one cell: lists of 1 and 2, two pairs, the single particle of the first list collides twice
    s = R.make_sheet([0.01, 0.02, 0.03], [0.01] * 3, [1.0] * 3, [0.1, -0.2, 0.05], [0.0, 0.1, -0.1], [1.0, 1.1, 0.9])
    log = R.collide(s, s, 2, 2, (0.0, 0.0), 0.1, 0.1, 0.1, -1.0, 1.0, background_density_SI=1e24, coulomb_log=10.0)
    assert log["visited"] == [(0, 1), (0, 2)] and log["pairs"] == 2
    # seven: lists of 3 and 4, four pairs, the first entry of the shuffled first list twice
    s, lo, dx = R.thermal_cells(2)
    cells = R.cell_lists(s, R.NX, R.NY, lo, dx, dx)
    seven = [c for c, l in cells.items() if len(l) == 7][0]
    keep = np.zeros(len(s["x"]), dtype=np.int32)
    keep[cells[seven]] = 1
    s["valid"] = keep
    log = _collide(s, lo, dx, False)
    first = [a for a, _ in log["visited"]]
    assert len(log["visited"]) == 4 and first[3] == first[0] and len(set(first)) == 3
    assert sorted(b for _, b in log["visited"]) == sorted(set(cells[seven]) - set(first))


def test_single_particle_and_cold_cells_are_untouched():
    # cell 0: one particle; cell 1: four cold particles (u = 0: no relative momentum); cell 2: two identical warm particles
    x = [0.01, 0.11, 0.12, 0.13, 0.14, 0.21, 0.22]
    ux = [0.3, 0.0, 0.0, 0.0, 0.0, 0.2, 0.2]
    psi = [0.8, 1.0, 1.0, 1.0, 1.0, 1.1, 1.1]
    s = R.make_sheet(x, [0.01] * 7, [1.0] * 7, ux, [0.0] * 7, psi)
    before = R.copy_sheet(s)
    log = R.collide(s, s, 4, 1, (0.0, 0.0), 0.1, 0.1, 0.1, -1.0, 1.0, background_density_SI=1e24)
    assert log["pairs"] == 0
    for k in ("ux", "uy"):
        assert np.array_equal(s[k], before[k]), k
    assert np.array_equal(s["psi"][:5], before["psi"][:5])
    # (the reference rewrites psi = gamma - uz / c of every pair it visits: a rounding of the warm pair's psi, nothing more)
    assert np.abs(s["psi"][5:] - before["psi"][5:]).max() <= 4 * np.finfo(float).eps


def test_unequal_weights_exercise_both_rejections():
    s, lo, dx = R.thermal_cells(4)
    log = _collide(s, lo, dx, False)
    assert log["rejected"][0] > 0 and log["rejected"][1] > 0


def _header():
    return open(os.path.join(ROOT, "include", "hpslice.h")).read()


def test_header_declares_the_collision_entry_points_and_lib_carries_them():
    hdr = _header()
    for name in ("hps_collide_plasma", "hps_engine_add_collision", "hps_engine_collision_stats"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib._SIGS, name
    assert len(_lib._SIGS["hps_collide_plasma"][1]) == 22
    assert len(_lib._SIGS["hps_engine_add_collision"][1]) == 5


# the members of hps_deck as of the commit before collisions: the feature is configured through a setter, not the deck
DECK_MEMBERS = """nx ny nz lo hi order deriv_type plasma_ppc plasma_density plasma_radius plasma_charge plasma_mass max_qsa n_subcycles
beam_profile beam_zmin beam_zmax beam_radius beam_density beam_umean beam_pos_mean beam_pos_std beam_ppc beam_charge bc mg_tol_rel
mg_tol_abs deposit_rho n_steps dt beam_n_subcycles beam_mass ext_E_slope bxby_solver predcorr_tol predcorr_max_iter predcorr_mix
field_bc laser_on laser_a0 laser_w0 laser_L0 laser_lambda0 laser_pos laser_zfoc laser_solver laser_use_phase si_units grid_current_on
grid_current_peak grid_current_mean grid_current_std laser_mg_tol_rel laser_mg_tol_abs beam_radiation_reaction background_density_SI
beam_no_z_push plasma_no_neutralize ion_on ion_ppc ion_density ion_mass ion_charge ion_init_level ion_Z ion_energies ion_seed
beam_spin_tracking beam_initial_spin beam_spin_anom dt_adaptive nt_per_betatron dt_max adaptive_threshold_uz adaptive_phase_tolerance
adaptive_no_predict_step adaptive_no_phase_control adaptive_phase_substeps adaptive_density max_time beam_uz_std ext_Ez_slope
beam_do_salame salame_n_iter salame_relative_tolerance salame_no_advance salame_Ez_target_slope""".split()


def test_deck_struct_is_unchanged():
    hdr = _header()
    body = hdr[:hdr.index("} hps_deck;")].rsplit("typedef struct {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        decl = re.sub(r"^(unsigned long long|double|int)\s+", "", stmt)
        names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(",")]
    assert names == DECK_MEMBERS
    assert [n for n, _ in _lib.Deck._fields_] == DECK_MEMBERS


def test_collisions_deck_is_the_blowout_SI_deck_plus_the_entry():
    d, base = decks.collisions_SI(), decks.blowout_wake_SI()
    assert d.pop("collisions") == [(0, 0, -1.0, 0)]
    assert d == base
    assert decks.collisions_SI(coulomb_log=5.0, seed=3)["collisions"] == [(0, 0, 5.0, 3)]
    # fill_struct skips the entry: the struct of the deck is the struct of the blowout deck
    a, b = _lib.fill_struct(_lib.Deck(), decks.collisions_SI()), _lib.fill_struct(_lib.Deck(), base)
    assert bytes(a) == bytes(b)
