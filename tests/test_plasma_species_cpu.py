"""Further plasma species without a GPU: the deck entry's validation, name -> index resolution, and the adaptive time step's
rho_max over three species (hps_adaptive_add_species) against numpy."""
import ctypes as C

import numpy as np
import pytest

from hipace_amd import decks


# ---- decks.plasma_species ---------------------------------------------------------------------------------------------------
def _deck(*species):
    return dict(decks.blowout_wake(), plasma_species=list(species))


H = dict(name="H_ion", charge=1.0, mass=1836.0, density=1.0)


def test_valid_entry_over_the_defaults():
    (s,) = decks.plasma_species(_deck(dict(H, ppc=(2, 1), temperature_in_ev=10.0)))
    assert s["name"] == "H_ion"
    assert s["record"] == dict(charge=1.0, mass=1836.0, density=1.0, ppc=(2, 1), fine_ppc=(0, 0), neutralize_background=1)
    # u_std = sqrt(T q_e / (M c^2)), the mass in electron masses in a normalised deck (decks.thermal_u_std)
    ref = (10.0 * 1.602176634e-19 / (1836.0 * 9.1093837015e-31 * 299792458.0 ** 2)) ** 0.5
    assert s["u_std"] == (ref,) * 3 and s["u_mean"] == (0.0, 0.0, 0.0) and s["density"] is None
    assert set(decks.PLASMA_SPECIES_DEFAULT) == {"name", "charge", "mass", "density", "ppc", "fine_ppc", "neutralize_background", "u_mean",
                                                 "u_std", "temperature_in_ev", "seed", "density_expr", "density_table",
                                                 "density_constants", "min_density"}
    assert decks.PLASMA_SPECIES_DEFAULT["neutralize_background"] is True
    assert decks.plasma_species(decks.blowout_wake()) == []
    # the charge defaults to the opposite of the plasma's
    assert decks.plasma_species(_deck(dict(mass=2.0, density=1.0)))[0]["record"]["charge"] == 1.0
    (t,) = decks.plasma_species(_deck(dict(H, density_table=[(0.0, "1"), (2.0, "2*x")], min_density=0.5)))
    assert t["density"] == ([(0.0, "1"), (2.0, "2*x")], None, 0.5)


@pytest.mark.parametrize("entry, needle", [
    ([dict(H, colour="red")], "unknown entries ['colour']"),
    ([dict(H), dict(H, mass=2.0)], "a name is given twice"),
    ([dict(H, name=f"s{k}") for k in range(5)], "at most 4 species"),
    ([dict(name="x", charge=1.0, mass=1.0)], "density is required"),
    ([dict(name="x", charge=1.0, density=1.0)], "mass is required"),
    ([dict(H, name="ion")], "belongs to species 1"),
    ([dict(H, u_std=(0.1, 0.1, 0.1), temperature_in_ev=5.0)], "exclusively"),
    ([dict(H, density_expr="1", density_table=[(0.0, "1")])], "not both"),
    ([dict(H, min_density=0.1)], "min_density needs"),
    (dict(H), "a list of dicts"),
])
def test_refused_entries(entry, needle):
    with pytest.raises(ValueError) as err:
        decks.plasma_species(dict(decks.blowout_wake(), plasma_species=entry))
    assert needle in str(err.value), str(err.value)


def test_name_to_index_resolution():
    deck = _deck(dict(H), dict(mass=3.0, density=0.5), dict(H, name="He"))
    names = decks.plasma_species_names(deck)
    assert names == ["plasma", "ion", "H_ion", "species3", "He"]
    for k, n in enumerate(names):
        assert decks.plasma_species_index(names, n) == k == decks.plasma_species_index(names, k)
    with pytest.raises(ValueError, match="no plasma species named 'electrons'"):
        decks.plasma_species_index(names, "electrons")
    with pytest.raises(ValueError, match="no plasma species 5"):
        decks.plasma_species_index(names, 5)
    d3 = decks.blowout_wake_three_species()
    assert decks.plasma_species_names(d3) == ["plasma", "ion", "H_ion"] and d3["ion_on"] == 1 and d3["plasma_no_neutralize"] == 1
    assert (d3["nx"], d3["ny"], d3["nz"]) == (64, 64, 24)


# ---- hps_adaptive_add_species ---------------------------------------------------------------------------------------------------
def _adaptive_deck(**kw):
    d = decks.adaptive_time_step()
    d.update(plasma_ppc=(1, 1), plasma_density=1.0, adaptive_density=0.25, **kw)
    decks.with_ion_species(d, "H", 0.8, ppc=(1, 1), initial_level=1)
    d["background_density_SI"] = 1.0e24
    return d


CT, FT = (0.0, 4.0, 8.0), (1.0, 1.5, 0.5)                 # the tabulated profile's time factor f_t(c t)
TABLE = [(2.0, "0.3 + 0.1*z"), (6.0, "2.0 - 0.2*z")]      # species 1: a density table, lower_bound in z
EXPR3, Q3, N3 = "n3*(1 + 0.5*sin(z))", 2.0, 0.9           # species 2: a parsed density, charge 2


def _reference(z, third):
    f_t = np.interp(z, CT, FT)
    r = [abs(0.25 * 1.0), abs(-1.0 * 1.0 * f_t)]                                  # |adaptive_density q_e|, the plasma: constant x table
    prog = TABLE[min(int(np.searchsorted([p for p, _ in TABLE], z, side="left")), len(TABLE) - 1)][1]
    r.append(abs(1.0 * eval(prog, {"z": z})))                                     # the ion: its table's entry in force
    if third:
        r.append(abs(Q3 * N3 * (1.0 + 0.5 * np.sin(z))))
    return max(r)


def test_rho_max_takes_the_maximum_over_three_species():
    from hipace_amd import _lib, api
    deck = _adaptive_deck(ion_density_table=TABLE)
    three = dict(deck, plasma_species=[dict(name="dopant", charge=Q3, mass=7.0, density=N3, density_expr=EXPR3,
                                            density_constants=dict(n3=N3))])
    a2 = api.AdaptiveTimeStep(deck, density_profile=((), (), CT, FT))
    a3 = api.AdaptiveTimeStep(three, density_profile=((), (), CT, FT))
    assert a3.plasma_species_names == ["plasma", "ion", "dopant"]
    larger = 0
    for z in np.linspace(-1.0, 9.0, 41):
        v2, v3 = a2.rho_max(z), a3.rho_max(z)
        assert abs(v2 - _reference(z, False)) <= 1e-15 * abs(v2), (z, v2, _reference(z, False))
        assert abs(v3 - _reference(z, True)) <= 1e-15 * abs(v3), (z, v3, _reference(z, True))
        assert v3 >= v2
        larger += v3 > v2
    assert larger > 10                                       # without the third species the value is smaller
    # a constant further species: |q n f_r(0) f_t(z)|, the index is the next free one, a seventh species is refused
    k = a2.add_species(-3.0, 2.0, "heavy")
    assert k == 2 and abs(a2.rho_max(4.0) - 3.0 * 2.0 * 1.5) <= 1e-15 * 9.0
    for j in range(3):
        assert a2.add_species(1.0, 1.0e-3) == 3 + j
    with pytest.raises(_lib.HpsError, match="HPS_MAX_PLASMA_SPECIES"):
        a2.add_species(1.0, 1.0)
    assert _lib.lib().hps_adaptive_add_species(None, 1.0, 1.0) == -1
    with pytest.raises(_lib.HpsError, match="index of an added species"):
        api.AdaptiveTimeStep(deck).set_density_expr(2, "1")
