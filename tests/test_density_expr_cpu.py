"""Parsed plasma densities without a device: the compiler on the reference's own density, the density table, the
adaptive time step's rho_max with programs, and the deck keys."""
import ctypes as C

import numpy as np
import pytest

from hipace_amd import _lib, decks, expr
from hipace_amd import api as A
from tests import density_expr_reference as D


def ulps(a, b):
    """distance in units of the last place of b"""
    return np.abs(a - b) / np.spacing(np.abs(b))


def adaptive_deck(**kw):
    d = decks.adaptive_time_step()
    d.update(plasma_ppc=(1, 1), plasma_density=2.0, plasma_charge=-1.0, adaptive_density=0.0)
    d.update(kw)
    return d


# ---- 1. the reference's own density ----------------------------------------------------------------------------------------

def test_lwfa_density_compiles_and_equals_the_closed_form():
    """examples/get_started/inputs_lwfa: the string with its line breaks and `if (`, the constants through one another; the
    host routine against the closed form in numpy, operation by operation in the string's order, to the 2 ulp of cos (8l)"""
    p = expr.compile_expr(decks.LWFA_DENSITY, ("x", "y", "z"), decks.LWFA_CONSTANTS)
    assert p.variables == ("x", "y", "z") and "cos" in [o for o, _ in p.ins]
    P = expr.PREDEFINED
    ne, Lramp = 1.0505e23, 6.0e-3
    wp = np.sqrt(ne * (P["q_e"] * P["q_e"]) / (P["m_e"] * P["epsilon0"]))
    kp_inv, kp = P["clight"] / wp, wp / P["clight"]
    Rm = 3.0 * kp_inv
    xs = np.linspace(-18.0 * kp_inv, 18.0 * kp_inv, 64)
    x, y = np.meshgrid(xs, xs)
    Rm2 = Rm * Rm
    for z in (-1e-3, 0.0, 3e-3, 6e-3, 7e-3):
        got = D.host_value(p, x, y, z)
        chan = ne * (1.0 + 4.0 * (x * x + y * y) / ((kp * kp) * (Rm2 * Rm2)))
        ramp = 1.0 if z > Lramp else 0.5 * (1.0 - np.cos(np.pi * z / Lramp))
        want = chan * ramp * (1.0 if z > 0.0 else 0.0)
        assert got.shape == want.shape
        if z <= 0.0:
            assert np.all(got == 0.0)
        else:
            assert ulps(got, want).max() <= 2.0, (z, ulps(got, want).max())
    assert np.array_equal(D.host_value(p, x, y, 7e-3), p.evaluate(x, y, np.full(x.shape, 7e-3)))      # arithmetic only beyond the ramp


def test_an_expression_that_names_t_is_refused():
    with pytest.raises(ValueError, match=r"unknown name: 't'"):
        expr.compile_density("1 + 0.1*t")
    with pytest.raises(ValueError, match=r"unknown name: 't'"):
        expr.compile_density([(0.0, "1"), (1.0, "x + t")])


def test_line_breaks_and_if_with_a_blank():
    a = expr.compile_expr("1 +\n  if (x > 0,\n 2, 3) *\ty", ("x", "y", "z"))
    b = expr.compile_expr("1 + if(x > 0, 2, 3) * y", ("x", "y", "z"))
    assert a.ins == b.ins and a.consts == b.consts


# ---- 2. the density table --------------------------------------------------------------------------------------------------

def test_density_table_file_and_lower_bound(tmp_path):
    path = tmp_path / "table.txt"
    path.write_text("3.0 2\n1.0   1\n\nnot a line\n5.0 3\n3.0 7\n")
    table = decks.read_density_table(str(path))
    assert table == [(1.0, "1"), (3.0, "2"), (5.0, "3")]      # std::map: sorted, the first of two equal positions stays
    ats = A.AdaptiveTimeStep(adaptive_deck(plasma_density_table=str(path)))
    # lower_bound: the first entry with position >= z, the last one beyond the table
    for z, want in ((-2.0, 1.0), (0.999, 1.0), (1.0, 1.0), (1.5, 2.0), (3.0, 2.0), (3.0000001, 3.0), (5.0, 3.0), (9.0, 3.0)):
        assert ats.rho_max(z) == want, z
    with pytest.raises(ValueError, match="unable to get any data"):
        empty = tmp_path / "empty.txt"
        empty.write_text("\n# nothing\n")
        decks.read_density_table(str(empty))


# ---- 3. rho_max --------------------------------------------------------------------------------------------------------------

def test_rho_max_with_a_program_is_bit_equal_to_numpy():
    n0, q = 1.7, -1.0
    ats = A.AdaptiveTimeStep(adaptive_deck(plasma_charge=q), density_exprs={0: ("n0*(1 + z/8)", dict(n0=n0))})
    z = np.linspace(-3.0, 40.0, 10)
    got = np.array([ats.rho_max(v) for v in z])
    want = np.abs(q * (n0 * (1.0 + z / 8.0)))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_rho_max_takes_the_larger_species_and_adaptive_density():
    d = adaptive_deck(plasma_density=1.0)
    decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=1)
    ats = A.AdaptiveTimeStep(d, density_exprs={0: ("1 + 0.5*z", None), 1: ("4 - z", None)})
    assert ats.rho_max(0.0) == 4.0 and ats.rho_max(1.0) == 3.0 and ats.rho_max(2.0) == 2.0 and ats.rho_max(3.0) == 2.5
    assert ats.rho_max(5.0) == 3.5                      # |charge * value|: the ions' -1 counts as 1, the plasma's 3.5 wins
    assert ats.rho_max(10.0) == 6.0 and ats.rho_max(20.0) == 16.0
    ats = A.AdaptiveTimeStep(dict(d, adaptive_density=5.0), density_exprs={0: ("1 + 0.5*z", None), 1: ("4 - z", None)})
    assert ats.rho_max(0.0) == 5.0 and ats.rho_max(10.0) == 6.0
    # a program on one species only: the other keeps density f_r(0) f_t(z)
    ats = A.AdaptiveTimeStep(d, density_profile=((), (), (0.0, 4.0), (0.25, 1.0)), density_exprs={1: ("0.1", None)})
    assert ats.rho_max(0.0) == 0.25 and ats.rho_max(2.0) == 0.625 and ats.rho_max(8.0) == 1.0


def test_rho_max_without_programs_is_the_tables():
    d = adaptive_deck(plasma_density=2.0)
    ats = A.AdaptiveTimeStep(d, density_profile=((0.0, 1.0), (1.5, 3.0), (0.0, 4.0), (0.25, 1.0)))
    for z, ft in ((-1.0, 0.25), (0.0, 0.25), (2.0, 0.625), (4.0, 1.0), (7.0, 1.0)):
        assert ats.rho_max(z) == abs(-1.0 * 2.0 * (1.5 * ft)), z
    assert A.AdaptiveTimeStep(d).rho_max(3.0) == 2.0


def test_adaptive_setter_refusals():
    ats = A.AdaptiveTimeStep(adaptive_deck())
    with pytest.raises(_lib.HpsError, match="no ion species"):
        ats.set_density_expr(1, "1")
    with pytest.raises(_lib.HpsError, match="strictly ascending"):
        ats.set_density_expr(0, [(2.0, "1"), (2.0, "2")])
    bad = expr.Program([("var", 3)], [], ("x", "y", "z", "t"))
    with pytest.raises(_lib.HpsError, match="variable index beyond n_vars"):
        ats.set_density_expr(0, bad)
    with pytest.raises(_lib.HpsError, match="n_progs must be >= 1"):
        _lib.check(_lib.lib().hps_adaptive_set_density_expr(ats._h, 0, 0, None, None))
    assert ats.rho_max(1.0) == 2.0                      # a refusal leaves the controller as it was


# ---- 4. the deck keys --------------------------------------------------------------------------------------------------------

def test_deck_keys():
    assert decks.DENSITY_EXPR_DEFAULT == dict(plasma_density_expr=None, ion_density_expr=None, plasmas_density_expr=None,
                                              plasma_min_density=None, ion_min_density=None, plasma_density_table=None,
                                              ion_density_table=None, density_constants=None)
    d = decks.blowout_wake()
    assert decks.density_exprs(d) == {}
    d.update(decks.DENSITY_EXPR_DEFAULT)
    assert decks.density_exprs(d) == {}                 # a deck without them makes no call
    decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=1)
    d.update(plasmas_density_expr="1 + a*x", density_constants=dict(a=0.1), ion_density_expr="2", ion_min_density=0.5)
    got = decks.density_exprs(d)
    assert got == {0: ("1 + a*x", dict(a=0.1), 0.0), 1: ("2", dict(a=0.1), 0.5)}      # the shared form; a species' own key wins
    d.update(plasma_density_table=[(0.0, "1"), (2.0, "3")], plasmas_density_expr=None)
    assert decks.density_exprs(d)[0] == ([(0.0, "1"), (2.0, "3")], dict(a=0.1), 0.0)
    with pytest.raises(ValueError, match="not both"):
        decks.density_exprs(dict(d, plasma_density_expr="1"))
    with pytest.raises(ValueError, match="not both"):
        decks.density_exprs(dict(d, ion_density_table=[(0.0, "1")]))
    with pytest.raises(ValueError, match="min_density needs"):
        decks.density_exprs(dict(decks.blowout_wake(), plasma_min_density=0.1))
    with pytest.raises(ValueError, match="no ion species"):
        decks.density_exprs(dict(decks.blowout_wake(), ion_density_expr="1"))


def test_production_lwfa_parsed_deck():
    d = decks.production_lwfa_parsed()
    tab, prof = decks.production_lwfa()
    assert {k: v for k, v in d.items() if k not in decks.DENSITY_EXPR_DEFAULT} == tab
    spec = decks.density_exprs(d)
    assert set(spec) == {0} and spec[0][0] == decks.LWFA_DENSITY and "\n" in spec[0][0] and spec[0][2] == 0.0
    assert all(isinstance(spec[0][1][k], str) for k in ("wp", "kp", "kp_inv", "Rm"))
    # the program on the lattice's own radii and the steps' own times against the tables of production_lwfa(): the same function
    r, fr, ct, ft = prof
    progs, pos = expr.compile_density(spec[0][0], spec[0][1])
    assert pos is None and len(progs) == 1
    for k in (0, 1, 5, 10):
        got = D.host_value(progs[0], r, np.zeros_like(r), ct[k])
        want = tab["plasma_density"] * fr * ft[k]
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_c_int_signature_of_the_new_entries():
    L = _lib.lib()
    for name in ("hps_engine_set_density_expr", "hps_adaptive_set_density_expr", "hps_adaptive_rho_max"):
        assert name in _lib._SIGS and getattr(L, name).restype is C.c_int
