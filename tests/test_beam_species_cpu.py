"""Several beam species in one engine, the parts that need no GPU: the deck entry beam_species and its refusals, the
numpy merge the GPU tests compare the container with, and the adaptive controller over several beams
(hps_adaptive_initial_dt_beams / hps_adaptive_after_step_beams, AdaptiveTimeStep.cpp:94-110, 177-258)."""
import ctypes as C

import numpy as np
import pytest

from hipace_amd import decks
from tests import beam_species_reference as S


# ---- 1. the deck entry ------------------------------------------------------------------------------------------------------
FW = dict(num_particles=100, position_mean=(0.0, 0.0, 0.0), position_std=(0.1, 0.1, 0.2), u_mean=(0.0, 0.0, 50.0), u_std=(0.0, 0.0, 2.0),
          density=1.0)


def test_entry_takes_the_decks_constants_and_the_sources_uz():
    d = dict(decks.beam_evolution(), beam_charge=-1.0, beam_mass=3.0, beam_n_subcycles=6, beam_no_z_push=1)
    assert decks.beam_species(d) == []
    d["beam_species"] = [dict(name="witness", fixed_weight=FW), dict(charge=1.0, mass=2.0, do_z_push=True, n_subcycles=3,
                                                                    particles=np.zeros((7, 5)), uz_mean=7.0, uz_std=0.5)]
    a, b = decks.beam_species(d)
    assert a["name"] == "witness" and a["source"] == "fixed_weight" and a["args"]["num_particles"] == 100
    assert a["args"]["seed"] == decks.BEAM_FIXED_WEIGHT_DEFAULT["seed"]
    assert a["record"] == dict(charge=-1.0, mass=3.0, n_subcycles=6, no_z_push=1, radiation_reaction=0, do_spin_tracking=0,
                               spin_anom=d.get("beam_spin_anom", 0.0), uz_mean=50.0, uz_std=2.0)
    assert b["name"] is None and b["source"] == "particles" and b["args"]["soa"].shape == (7, 5)
    assert (b["record"]["charge"], b["record"]["mass"], b["record"]["n_subcycles"], b["record"]["no_z_push"]) == (1.0, 2.0, 3, 0)
    assert (b["record"]["uz_mean"], b["record"]["uz_std"]) == (7.0, 0.5)
    e = decks.beam_species_spec(d, dict(density_expr="exp(-x^2)", u_std=(0.1, 0.1, 0.2), seed=4))
    assert e["source"] == "density_expr" and e["args"] == dict(expr="exp(-x^2)", constants=None, min_density=0.0, u_std=(0.1, 0.1, 0.2),
                                                              random_ppc=(0, 0, 0), seed=4)


@pytest.mark.parametrize("entry, message", [
    ([dict(fixed_weight=FW, colour="red")], "unknown entries \\['colour'\\]"),
    ([dict(name="w")], "exactly one source"),
    ([dict(fixed_weight=FW, particles=np.zeros((7, 1)))], "exactly one source"),
    ([dict(fixed_weight=dict(FW, sigma=1.0))], "fixed_weight: unknown entries \\['sigma'\\]"),
    ([dict(fixed_weight_pdf=dict(pdf="1", num_particle=4))], "fixed_weight_pdf: unknown entries \\['num_particle'\\]"),
    ([dict(particles=np.zeros((6, 3)))], "\\(7, n\\) array"),
    ([dict(particles=[1.0, 2.0])], "\\(7, n\\) array"),
    ([dict(fixed_weight=FW, min_density=0.1)], "min_density go with density_expr"),
    ([dict(fixed_weight=FW)] * 4, "at most 3 species"),
    ([dict(name="w", fixed_weight=FW), dict(name="w", fixed_weight=FW)], "a name is given twice"),
    (dict(fixed_weight=FW), "a list of dicts"),
])
def test_bad_entries_raise_value_error(entry, message):
    with pytest.raises(ValueError, match=message):
        decks.beam_species(dict(decks.beam_evolution(), beam_species=entry))


def test_production_pwfa_deck_parses_and_its_species_validate():
    from hipace_amd import _lib
    d = decks.production_pwfa(seed=3)
    assert (d["nx"], d["ny"], d["nz"], d["n_steps"]) == (64, 64, 100, 11) and d["dt_adaptive"] == 1 and d["nt_per_betatron"] == 30.0
    assert d["max_time"] == 0.3 / decks.SI["c"] and d["ion_on"] == 1 and d["plasma_no_neutralize"] == 1 and d["si_units"] == 1
    _lib.fill_struct(_lib.Deck(), d)                               # every member of hps_deck it names takes its value
    assert decks.beam_fixed_weight(d)["total_charge"] == 0.6e-9 and decks.beam_fixed_weight(d)["seed"] == 3
    (w,) = decks.beam_species(d)
    assert w["name"] == "witness" and w["source"] == "fixed_weight" and w["args"]["total_charge"] == 0.2e-9
    assert w["args"]["do_symmetrize"] and w["args"]["position_mean"][2] == -160.0 * 1.0e-6 and w["args"]["seed"] == 1003
    assert w["record"]["charge"] == d["beam_charge"] and w["record"]["mass"] == d["beam_mass"]
    assert (w["record"]["uz_mean"], w["record"]["uz_std"]) == (1000.0, 10.0)
    assert decks.production_pwfa(nxy=32, nz=20, n_steps=2)["nz"] == 20


# ---- 2. the numpy merge -----------------------------------------------------------------------------------------------------
def test_merge_by_hand():
    """4 slices of dz = 1 from z = 0; slice p from the head holds z in [3 - p, 4 - p)"""
    a = np.zeros((7, 4)); a[2] = [3.5, 0.2, 3.1, 9.0]; a[6] = [1, 2, 3, 4]           # 9.0: outside
    b = np.zeros((7, 3)); b[2] = [0.7, 3.9, 2.5]; b[6] = [10, 20, 30]
    c = np.zeros((7, 2)); c[2] = [-0.5, 3.0]; c[6] = [100, 200]                      # -0.5: the cast's slice 0
    B, soa, tags, counts = S.merge([a, b, c], 0.0, 1.0, 4)
    assert B.tolist() == [0, 4, 5, 5, 8] and counts == [3, 3, 2]
    assert soa[6].tolist() == [1, 3, 20, 200, 30, 2, 10, 100]
    assert tags.tolist() == [0, 0, 1, 2, 1, 0, 1, 2]
    one = S.merge([a], 0.0, 1.0, 4)
    assert one[0].tolist() == [0, 2, 2, 2, 3] and one[1][6].tolist() == [1, 3, 2] and not one[2].any()


def test_the_shared_beams_hold_the_shapes_the_kernels_can_go_wrong_at():
    sp = S.three_species()
    B, soa, tags, counts = S.merge([s for _, s in sp], -2.4, 0.4, 12)
    per = np.diff(B)
    assert counts == [333, 2600, 150] and per.max() > 2048 and (per == 0).sum() >= 2 and tags.max() == 2
    only_a = [p for p in range(12) if per[p] and set(tags[B[p]:B[p + 1]]) == {0}]
    assert only_a, "no slice that holds one species alone"
    assert len(set(soa[6])) == soa.shape[1], "the weights are the particles' fingerprints"
    slow = sp[2][1][5] < 0.2      # u_z = 0.1: 0.9 (1 - 0.0995) = 0.81 backwards per step, two slices of 0.4
    assert slow.sum() == 12 and 0.9 * (1.0 - 0.1 / np.sqrt(1.01)) > 2 * 0.4


# ---- 3. the controller over several beams -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hipace_amd import _lib
    return _lib.lib()


def _arr(v):
    a = np.ascontiguousarray(v, dtype=np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


def _after_beams(lib, ats, moments, charge, mass, t, nstages=1):
    from hipace_amd.api import check
    (m, pm), (q, pq), (ms, pms) = _arr(moments), _arr(charge), _arr(mass)
    dt = C.c_double()
    check(lib.hps_adaptive_after_step_beams(ats._h, len(q), pm, pq, pms, float(t), int(nstages), C.byref(dt)))
    return dt.value


def _initial_beams(lib, ats, uz_mean, uz_std, charge, mass, nstages=1):
    from hipace_amd.api import check
    (a, pa), (b, pb), (q, pq), (ms, pms) = _arr(uz_mean), _arr(uz_std), _arr(charge), _arr(mass)
    dt = C.c_double()
    check(lib.hps_adaptive_initial_dt_beams(ats._h, len(q), pa, pb, pq, pms, int(nstages), C.byref(dt)))
    return dt.value


MOMENTS = [np.array([2.0, 2.0 * 900.0, 2.0 * 900.0 ** 2 + 50.0, 880.0]), np.array([1.5, 1.5 * 700.0, 1.5 * 700.0 ** 2 + 90.0, 650.0]),
           np.array([3.0, 3.0 * 20.0, 3.0 * 20.0 ** 2 + 1.0, 1.5])]      # the last: below the threshold u_z of 2


@pytest.mark.parametrize("nstages", [1, 3])
def test_one_beam_through_the_beams_calls_is_the_one_beam_controller(lib, nstages):
    from hipace_amd.api import AdaptiveTimeStep
    d = decks.adaptive_time_step(+1)
    a, b = AdaptiveTimeStep(d), AdaptiveTimeStep(d)
    q, m = [d["beam_charge"]], [d["beam_mass"]]
    um, us = d["beam_umean"][2], d.get("beam_uz_std", 0.0)
    assert a.initial_dt(nstages=nstages) == _initial_beams(lib, b, [um], [us], q, m, nstages)
    t = 0.0
    for mom in MOMENTS + MOMENTS[:1]:
        da, db = a.CalculateFromDensity(t), b.CalculateFromDensity(t)
        assert da == db and da > 0.0
        assert a.CalculateFromMinUz(mom, t, nstages) == _after_beams(lib, b, [mom], q, m, t, nstages)
        assert a.next_time() == b.next_time()
        t = a.next_time()


def test_two_beams_take_the_smaller_dt_and_a_beam_of_charge_zero_is_skipped(lib):
    from hipace_amd.api import AdaptiveTimeStep
    base = dict(decks.adaptive_time_step(+1), adaptive_no_phase_control=1)
    light, heavy = dict(base, beam_charge=-1.0, beam_mass=1.0), dict(base, beam_charge=1.0, beam_mass=1836.0)
    one = {}
    for name, d in (("light", light), ("heavy", heavy)):
        c = AdaptiveTimeStep(d)
        c.initial_dt()
        c.CalculateFromDensity(0.0)
        one[name] = c.CalculateFromMinUz(MOMENTS[0], 0.0, 1)
    assert one["light"] < one["heavy"]
    both = AdaptiveTimeStep(base, beams=[dict(charge=-1.0, mass=1.0, uz_mean=900.0, uz_std=5.0), dict(charge=1.0, mass=1836.0, uz_mean=900.0, uz_std=5.0)])
    both.initial_dt()
    both.CalculateFromDensity(0.0)
    assert both.CalculateFromMinUz(np.stack([MOMENTS[0], MOMENTS[0]]), 0.0, 1) == one["light"]
    # ... the other way round, and with each beam's own moments: the smaller of the two one-beam answers
    swapped = AdaptiveTimeStep(base)
    swapped.initial_dt()
    swapped.CalculateFromDensity(0.0)
    assert _after_beams(lib, swapped, [MOMENTS[0], MOMENTS[0]], [1.0, -1.0], [1836.0, 1.0], 0.0) == one["light"]
    # a beam of charge 0 does not set dt, whatever its moments (not even none at all: sum w = 0): it keeps the dt that was
    # (new_dts[ibeam] = dt, AdaptiveTimeStep.cpp:188-191), which the minimum over the beams then sees
    for mom, other in ((MOMENTS[0], "heavy"), (MOMENTS[1], "light")):
        d = heavy if other == "heavy" else light
        alone, skip = AdaptiveTimeStep(d), AdaptiveTimeStep(d)
        dt0 = alone.initial_dt()
        assert skip.initial_dt() == dt0
        alone.CalculateFromDensity(0.0)
        skip.CalculateFromDensity(0.0)
        want = min(dt0, alone.CalculateFromMinUz(mom, 0.0, 1))
        got = _after_beams(lib, skip, [np.array([0.0, 0.0, 0.0, np.inf]), mom], [0.0, d["beam_charge"]], [1.0, d["beam_mass"]], 0.0)
        print(f"charge 0 beside the {other} beam: dt before {dt0}, the beam's own {want}, got {got}")
        assert got == want
    # ... and a controller of nothing but such beams keeps the dt it had
    none = AdaptiveTimeStep(base)
    dt0 = none.initial_dt()
    none.CalculateFromDensity(0.0)
    assert _after_beams(lib, none, [MOMENTS[0]], [0.0], [1.0], 0.0) == dt0
    with pytest.raises(RuntimeError, match="sum of all weights is 0"):
        _after_beams(lib, AdaptiveTimeStep(base), [np.array([0.0, 0.0, 0.0, np.inf])], [-1.0], [1.0], 0.0)
    with pytest.raises(RuntimeError, match="n and nstages must be >= 1"):
        _after_beams(lib, AdaptiveTimeStep(base), np.zeros((0, 4)), [], [], 0.0)


def test_the_smallest_min_uz_mq_over_the_beams_feeds_the_phase_control(lib):
    """CalculateFromDensity cuts dt by the phase advance of m_min_uz_mq: with a density step right behind t = 0 the controller of
    two beams must cut as the one-beam controller of the lighter beam does"""
    from hipace_amd.api import AdaptiveTimeStep
    base = dict(decks.adaptive_time_step(+1), adaptive_phase_tolerance=1.0e-5)
    profile = ((), (), (0.0, 1.0, 1.5, 1.0e9), (1.0, 1.0, 6.0, 6.0))
    light = AdaptiveTimeStep(dict(base, beam_charge=-1.0, beam_mass=1.0), profile)
    light.initial_dt()
    light.CalculateFromDensity(0.0)
    light.CalculateFromMinUz(MOMENTS[0], 0.0, 1)
    both = AdaptiveTimeStep(base, profile, beams=[dict(charge=1.0, mass=1836.0), dict(charge=-1.0, mass=1.0)])
    both.initial_dt(uz_mean=900.0, uz_std=5.0)
    both.CalculateFromDensity(0.0)
    both.CalculateFromMinUz(np.stack([MOMENTS[1], MOMENTS[0]]), 0.0, 1)
    t = light.next_time()
    cut = light.CalculateFromDensity(t)
    assert both.CalculateFromDensity(t) == cut
    # (the test bites: the heavier beam's own m/q advances the phase more slowly and keeps a longer step)
    heavy = AdaptiveTimeStep(dict(base, beam_charge=1.0, beam_mass=1836.0), profile)
    heavy.initial_dt()
    heavy.CalculateFromDensity(0.0)
    heavy.CalculateFromMinUz(MOMENTS[1], 0.0, 1)
    assert heavy.CalculateFromDensity(t) > cut
