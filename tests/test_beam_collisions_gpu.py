"""Beam-plasma Coulomb collisions on the GPU: the operator against the numpy restatement particle by particle, order
independence, conservation, the engine's placement, keys and time step, the static beam against the reference's checksum
file, the refusals, and several steps in flight."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from hipace_amd import decks
from tests import collision_beam_reference as B
from tests import collision_reference as R
from tests.collision_util import deviation, from_gpu, geometry, sheet_arrays, sheet_from, small_deck, to_gpu, write_thermal
from tests.test_beam_collisions_cpu import CONSERVATION_BOUND, conservation_cases, conservation_error

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# Largest deviation of the GPU operator from the numpy restatement over every particle of every case of B.CASES, measured on
# the MI355X -- plasma particles: |du| / rms(u of the cell), as tests/test_collisions_gpu.py; beam particles: |du| / |u| of the
# particle.  MEASURED_OPERATOR_DEVIATION is that number; asserted: ten times it, the margin 8f took.  The worst
# case is a plasma electron of heavy_norm_auto_all_branches: where 40 heavy beam particles share a cell with one electron, that
# electron scatters 40 times by wide angles, and every scattering passes the last one's rounding on through 1 / v_rel^3.  The
# heavy cases leave 2.1e-12 to 3.1e-12 on the plasma and 3.7e-15 to 1.5e-14 on the beam; the electron-beam cases (gamma = 2000,
# narrow angles) at most 2.0e-16 on either.
MEASURED_OPERATOR_DEVIATION = 3.14e-12
OPERATOR_BOUND = 10.0 * MEASURED_OPERATOR_DEVIATION


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()
    return A


def beam_to_gpu(api, b):
    return api.BeamSlice(B.beam_soa(b), nsub=b["nsub"])


def beam_deviation(b_ref, got, dup=None):
    """max over the beam's particles of |du| / |u|; the two members of an exactly duplicated pair are interchangeable: they are
    compared as a set"""
    ref = np.stack([b_ref["ux"], b_ref["uy"], b_ref["uz"]])
    got = got.copy()
    if dup is not None:
        i, j = dup
        if np.abs(got[:, i] - ref[:, i]).max() > np.abs(got[:, j] - ref[:, i]).max():
            got[:, [i, j]] = got[:, [j, i]]
    return (np.abs(got - ref).max(axis=0) / np.sqrt((ref ** 2).sum(axis=0))).max()


def run_gpu(api, name, b0, s0, lo, dx):
    k = B.CASES[name]
    qb, mb, qp, mp = B.case_species(k)
    gb, gs = beam_to_gpu(api, b0), to_gpu(api, s0)
    pairs, over = api.BeamPlasmaCollision(gb, gs, geometry(api, lo, dx, k["si"]), qb, mb, qp, mp, B.case_dt(k), coulomb_log=k["L"],
                                          background_density_SI=k.get("bg", 0.0), seed=77, collision=1, step=3, islice=5)
    return gb.numpy(), from_gpu(gs), pairs, over


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_operator_matches_the_numpy_restatement(api, name):
    b0, s0, b1, s1, log, lo, dx, dup = B.reference_case(name)
    k = B.CASES[name]
    for br in k.get("branches", ()):
        assert log["branch"][br] > 0, (name, log["branch"])
    assert log["rejected"][0] > 0 and log["rejected"][1] > 0          # unequal weights: both rejection draws decide
    soa, us, pairs, over = run_gpu(api, name, b0, s0, lo, dx)
    c = R.C_SI if k["si"] else 1.0
    dev_p = deviation(s1, us, c, lo, dx)
    dev_b = beam_deviation(b1, soa[3:6], dup)
    print(f"{name}: deviation beam {dev_b:.3e} plasma {dev_p:.3e} pairs {pairs} (numpy {log['pairs']}) overfull {over} branches {log['branch']}")
    assert pairs == log["pairs"]
    assert over >= 2                      # 7 + 64, 40 + 64 and the cell of 1500 do not fit the LDS stage
    # positions and weights are not written; particles that are in no cell come back bit for bit
    assert np.array_equal(soa[:3], B.beam_soa(b0)[:3]) and np.array_equal(soa[6], b0["w"])
    la = B.beam_cell_lists(b0, R.NX, R.NY, lo, dx, dx)
    inside = np.zeros(len(b0["x"]), dtype=bool)
    inside[[ip for l in la.values() for ip in l]] = True
    if k.get("spoil"):
        assert (~inside).sum() > 40
    assert np.array_equal(soa[3:6][:, ~inside], B.beam_soa(b0)[3:6][:, ~inside])
    assert dev_b <= OPERATOR_BOUND and dev_p <= OPERATOR_BOUND, (name, dev_b, dev_p)


def test_result_does_not_depend_on_the_order_of_beam_or_sheet(api):
    name = "heavy_norm_auto_all_branches"
    b0, s0, _, _, _, lo, dx, _ = B.reference_case(name)
    soa, us, pairs, _ = run_gpu(api, name, b0, s0, lo, dx)
    rng = np.random.default_rng(1)
    pb, ps = rng.permutation(len(b0["x"])), rng.permutation(len(s0["x"]))
    soa2, us2, pairs2, _ = run_gpu(api, name, {q: v[pb] for q, v in b0.items()}, {q: v[ps] for q, v in s0.items()}, lo, dx)
    assert pairs == pairs2
    assert np.array_equal(soa[:, pb], soa2)
    for q in range(3):
        assert np.array_equal(us[q][ps], us2[q])


def test_gpu_conserves_momentum_and_energy_per_cell(api):
    for name, b, s, lo, dx, si, (qb, mb, qp, mp), dt, kw in conservation_cases():
        gb, gs = beam_to_gpu(api, b), to_gpu(api, s)
        pairs, _ = api.BeamPlasmaCollision(gb, gs, geometry(api, lo, dx, si), qb, mb, qp, mp, dt, **kw)
        b1, s1 = B.make_beam(gb.numpy(), b["nsub"]), R.copy_sheet(s)
        s1["ux"], s1["uy"], s1["psi"] = from_gpu(gs)
        ep, ee = conservation_error(b, s, b1, s1, mb, mp, R.C_SI if si else 1.0, lo, dx)
        print(f"{name}: pairs {pairs} momentum {ep:.3e} energy {ee:.3e}")
        assert pairs > 300 and ep <= CONSERVATION_BOUND and ee <= CONSERVATION_BOUND, (name, ep, ee)


# ---- the engine --------------------------------------------------------------------------------------------------------
BG = 1.0e30      # dense enough for the beam's pairs to scatter visibly in one step


def moving_deck(**kw):
    """16 x 16 cells, 12 slices of the blowout deck, 2 x 2 ppc, hipace.dt = 1; the beam comes from moving_beam"""
    d = dict(decks.blowout_wake(), nx=16, ny=16, nz=12, lo=(-8.0, -8.0, -0.72), hi=(8.0, 8.0, 0.72), plasma_ppc=(2, 2), n_steps=3,
             dt=1.0, beam_profile=-1, beam_n_subcycles=4, background_density_SI=BG)
    d.update(kw)
    return d


def moving_beam(deck):
    """a random Gaussian beam (no two particles share a coordinate) slow enough to slip: u = (0, 0, 3) +- (0.1, 0.1, 0.3)"""
    return decks.fixed_weight_beam(deck, 12000, 3.0, (0.13, -0.07, 0.0), (0.3, 0.3, 1.41), u_mean=(0.0, 0.0, 3.0), u_std=(0.1, 0.1, 0.3), seed=3)


def match(a, b):
    """for every column of positions a (3, n) the column of b (3, n) next to it: a bijection, or the test fails"""
    assert a.shape == b.shape
    if a.shape[1] == 0:
        return np.zeros(0, dtype=np.int64)
    d2 = ((a[:, :, None] - b[:, None, :]) ** 2).sum(axis=0)
    idx = d2.argmin(axis=1)
    assert sorted(idx.tolist()) == list(range(a.shape[1])) and d2[np.arange(a.shape[1]), idx].max() <= (1e-9 * np.abs(a).max()) ** 2
    return idx


def _head_slice_twins(api, deck, beam, u_std, add):
    """(engine with the collisions that add(engine) configures, its twin without any): the beam set, thermal momenta written
    into the sheet behind begin_step, the head slice solved"""
    from hipace_amd import _lib
    engines = []
    for collide in (True, False):
        e = api.SliceEngine(deck, tile_size=0)
        e.set_beam_particles(beam, allow_outside=True)
        if collide:
            add(e)
        e.begin_step()
        e.sync()
        write_thermal(_lib.lib().hps_engine_plasma(e._h), 1, u_std)
        e.solve_slice(deck["nz"] - 1)
        e.sync()
        engines.append(e)
    return engines


def test_engine_collides_the_beam_slice_behind_its_push_with_the_slice_key_and_the_step_dt(api):
    from hipace_amd import _lib
    L = _lib.lib()
    deck = moving_deck()
    beam = moving_beam(deck)
    u_std = 0.05
    nz = deck["nz"]
    with_c, without = _head_slice_twins(api, deck, beam, u_std, lambda e: e.add_beam_collision(0, -1.0, 42))
    st = with_c.collision_stats()
    assert st["pairs_collided"] > 100
    _, off0 = with_c.beam_layout()
    bc, sc = with_c.beam_state()
    bp, sp = without.beam_state()
    assert np.array_equal(bc, bp) and bc[0] == 0
    stay, slipped = slice(bc[0], bc[1]), slice(bc[1], off0[1])
    assert bc[1] - bc[0] > 50 and off0[1] - bc[1] > 10                    # the head slice keeps particles and hands some on
    # the twin's slice and sheet through the free operator with the engine's key and the run's time step
    el_c, id_c, lev_c = sheet_arrays(api, L.hps_engine_plasma(with_c._h))
    el_p, _, _ = sheet_arrays(api, L.hps_engine_plasma(without._h))
    assert np.array_equal((id_c >> np.uint64(24)) & np.uint64((1 << 39) - 1), np.arange(1, len(id_c) + 1, dtype=np.uint64))
    geom = api.Geometry(deck["nx"], deck["ny"], deck["lo"][:2], deck["hi"][:2], (deck["hi"][2] - deck["lo"][2]) / nz, bc=deck["bc"])
    gb, gs = api.BeamSlice(sp[:, stay]), sheet_from(api, el_p, id_c, lev_c)
    pairs, _ = api.BeamPlasmaCollision(gb, gs, geom, deck["beam_charge"], deck["beam_mass"], deck["plasma_charge"], deck["plasma_mass"],
                                       deck["dt"] / B.omega_p(BG), coulomb_log=-1.0, background_density_SI=BG, seed=42, collision=0, step=0,
                                       islice=nz - 1)
    assert pairs == st["pairs_collided"]
    want = gb.numpy()
    m = match(want[:3], sc[:3, stay])                                      # (the partition places particles with atomics)
    got = sc[:, stay][:, m]
    dev_b = (np.abs(got[3:6] - want[3:6]).max(axis=0) / np.sqrt((want[3:6] ** 2).sum(axis=0))).max()
    scale = np.array([u_std, u_std, 0.05])[:, None]
    dev_p = (np.abs(np.stack(from_gpu(gs)) - el_c[8:]) / scale).max()
    # the collision did something to both species, and nothing to the particles that slipped on to the next slice
    mp = match(sp[:3, stay], sc[:3, stay])
    changed_b = (np.abs(sc[3:6, stay][:, mp] - sp[3:6, stay]).max(axis=0) / np.sqrt((sp[3:6, stay] ** 2).sum(axis=0))).max()
    changed_p = (np.abs(el_c[8:] - el_p[8:]) / scale).max()
    ms = match(sp[:3, slipped], sc[:3, slipped])
    slipped_dev = (np.abs(sc[3:6, slipped][:, ms] - sp[3:6, slipped]).max(axis=0) / np.sqrt((sp[3:6, slipped] ** 2).sum(axis=0))).max()
    print(f"engine against operator: beam {dev_b:.3e} plasma {dev_p:.3e}; pairs {pairs}; changed by the collision: beam {changed_b:.3e} "
          f"plasma {changed_p:.3e}; slipped particles, engine with against engine without: {slipped_dev:.3e}")
    assert changed_b > 1e2 * OPERATOR_BOUND and changed_p > 1e2 * OPERATOR_BOUND
    assert slipped_dev <= OPERATOR_BOUND
    assert dev_b <= OPERATOR_BOUND and dev_p <= OPERATOR_BOUND


@pytest.mark.parametrize("kinds", [("plasma", "beam"), ("beam", "plasma")], ids="_then_".join)
def test_engine_runs_a_list_that_holds_both_kinds_in_its_order(api, kinds):
    """One list with a same-species collision and a beam collision, in either order, on the head slice of the moving deck.  The
    two kinds share the engine's cell lists: the counters must be all zero again behind every fill pass, slot 0 holds the
    sheet's list for one kind and the beam's for the other, and its offsets are the gate of the beam collision's plasma
    passes.  The twin engine's sheet and kept beam slice go through the two free operators in the list's order, with the
    collision index by position, the engine's seeds and the head slice's key; engine and replay run the same kernels on the
    same particles, so this file's OPERATOR_BOUND holds as in the test above."""
    from hipace_amd import _lib
    L = _lib.lib()
    deck = moving_deck()
    beam = moving_beam(deck)
    u_std = 0.05
    nz = deck["nz"]
    seed = dict(plasma=42, beam=43)

    def add(e):
        for k in kinds:
            e.add_collision(0, 0, -1.0, seed[k]) if k == "plasma" else e.add_beam_collision(0, -1.0, seed[k])
    with_c, without = _head_slice_twins(api, deck, beam, u_std, add)
    st = with_c.collision_stats()
    _, off0 = with_c.beam_layout()
    bc, sc = with_c.beam_state()
    bp, sp = without.beam_state()
    assert np.array_equal(bc, bp) and bc[0] == 0
    stay, slipped = slice(bc[0], bc[1]), slice(bc[1], off0[1])
    assert bc[1] - bc[0] > 50 and off0[1] - bc[1] > 10
    el_c, id_c, lev_c = sheet_arrays(api, L.hps_engine_plasma(with_c._h))
    el_p, _, _ = sheet_arrays(api, L.hps_engine_plasma(without._h))
    geom = api.Geometry(deck["nx"], deck["ny"], deck["lo"][:2], deck["hi"][:2], (deck["hi"][2] - deck["lo"][2]) / nz, bc=deck["bc"])
    gb, gs = api.BeamSlice(sp[:, stay]), sheet_from(api, el_p, id_c, lev_c)
    pairs = {}
    for i, k in enumerate(kinds):
        key = dict(coulomb_log=-1.0, background_density_SI=BG, seed=seed[k], collision=i, step=0, islice=nz - 1)
        if k == "plasma":
            pairs[k], _ = api.CoulombCollision(gs, gs, geom, deck["plasma_charge"], deck["plasma_mass"], **key)
        else:
            pairs[k], _ = api.BeamPlasmaCollision(gb, gs, geom, deck["beam_charge"], deck["beam_mass"], deck["plasma_charge"],
                                                  deck["plasma_mass"], deck["dt"] / B.omega_p(BG), **key)
    # 4 particles per cell over 256 cells, and the beam pairs the test above requires of this deck: both kinds have work
    assert pairs["plasma"] > 100 and pairs["beam"] > 100, pairs
    assert st["pairs_collided"] == pairs["plasma"] + pairs["beam"]
    want = gb.numpy()
    m = match(want[:3], sc[:3, stay])
    got = sc[:, stay][:, m]
    dev_b = (np.abs(got[3:6] - want[3:6]).max(axis=0) / np.sqrt((want[3:6] ** 2).sum(axis=0))).max()
    scale = np.array([u_std, u_std, 0.05])[:, None]
    dev_p = (np.abs(np.stack(from_gpu(gs)) - el_c[8:]) / scale).max()
    ms = match(sp[:3, slipped], sc[:3, slipped])
    slipped_dev = (np.abs(sc[3:6, slipped][:, ms] - sp[3:6, slipped]).max(axis=0) / np.sqrt((sp[3:6, slipped] ** 2).sum(axis=0))).max()
    print(f"{kinds}: engine against operators: beam {dev_b:.3e} plasma {dev_p:.3e}; pairs {pairs}, engine {st}; slipped particles, "
          f"engine with against engine without: {slipped_dev:.3e}")
    assert slipped_dev <= OPERATOR_BOUND
    assert dev_b <= OPERATOR_BOUND and dev_p <= OPERATOR_BOUND


def _head_slice_state(api, deck, collide):
    e = api.SliceEngine(deck, tile_size=0)
    if collide:
        e.add_beam_collision(0, -1.0, 1)
    e.set_diagnostics(True)
    e.begin_step()
    e.solve_slice(deck["nz"] - 1)
    e.solve_slice(deck["nz"] - 2)
    real, _ = e.particles()
    return real, e.slab(), e.checksums(), (e.collision_stats() if collide else None)


def test_beam_collision_on_slices_without_beam_particles_changes_nothing(api):
    """A moving beam that starts below the two head slices: no beam particle, no pair, no change.  The rule of
    test_engine_without_pairs_is_the_engine_without_collisions: two plain runs are compared first; where they agree bit for
    bit the run with the collision must too, otherwise 1e-9 of the largest entry is asserted."""
    deck = dict(decks.blowout_wake(), n_steps=1, dt=1.0, beam_zmax=5.0, background_density_SI=1.0e24)
    r0, s0, c0, _ = _head_slice_state(api, deck, False)
    r1, s1, c1, _ = _head_slice_state(api, deck, False)
    r2, s2, c2, st = _head_slice_state(api, deck, True)
    assert st == dict(pairs_collided=0, overfull_cells=0)
    if np.array_equal(r0, r1) and np.array_equal(s0, s1):
        assert np.array_equal(r0, r2) and np.array_equal(s0, s2) and c0 == c2
    else:
        print("two plain runs differ in rounding: asserting the engine-against-engine bound")
        for a, b in ((r0, r2), (s0, s2)):
            assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()


def test_static_beam_collides_nothing_and_holds_the_reference_checksums(api):
    """tests/collisions_beam.SI.1Rank.sh: hipace.dt = 0, so the reference's collision leaves rounding only and the engine
    launches nothing.  Every lev=0 entry within 5e-9 of the file (about five times what the collision-free oracle leaves, thirty
    times below the distance to the plasma-plasma file), the beam block within 1e-9."""
    gold = json.load(open(os.path.join(GOLD, "collisions_beam.SI.1Rank.json")))
    e = api.SliceEngine(decks.collisions_beam_SI(), tile_size=0)
    e.set_diagnostics(True)
    e.run_step()
    cs = e.checksums()
    assert e.collision_stats() == dict(pairs_collided=0, overfull_cells=0)
    bad = []
    for k, v in gold["lev=0"].items():
        dev = abs(cs[k] - v)
        print(f"{k}: file {v:.10e} engine {cs[k]:.10e} deviation/|v| {dev / max(abs(v), 1e-300):.2e}")
        if dev > 5e-9 * abs(v):
            bad.append(k)
    _, soa = e.beam_state()
    gb = gold["beam"]
    mine = dict(x=np.abs(soa[0]).sum(), y=np.abs(soa[1]).sum(), z=np.abs(soa[2]).sum(), ux=np.abs(soa[3]).sum() / R.C_SI,
                uy=np.abs(soa[4]).sum() / R.C_SI, uz=np.abs(soa[5]).sum() / R.C_SI, w=np.abs(soa[6]).sum())
    for k, v in mine.items():
        print(f"beam {k}: {v:.10e} file {gb[k]:.10e}")
        if abs(v - gb[k]) > 1e-9 * abs(gb[k]):
            bad.append("beam " + k)
    assert not bad, bad


def test_refusals(api):
    from hipace_amd._lib import HpsError

    def refused(deck, args, status, text, begin=False):
        e = api.SliceEngine(deck, tile_size=0)
        if begin:
            e.begin_step()
        with pytest.raises(HpsError) as err:
            e.add_beam_collision(*args)
        assert f"status {status}:" in str(err.value) and text in str(err.value), str(err.value)
    small = small_deck(decks.blowout_wake(), dt=1.0)
    dense = dict(small, background_density_SI=1e24)
    refused(small, (0, -1.0, 0), 1, "background_density_SI")
    refused(dense, (1, -1.0, 0), 1, "ion_on")
    refused(dense, (2, -1.0, 0), 1, "is 0 (plasma) or 1 (ion)")
    refused(dense, (0, -1.0, 0), 1, "before the first hps_engine_begin_step", begin=True)
    refused(small_deck(decks.ionization_SI(), plasma_ppc=(0, 0)), (1, -1.0, 0), 7, "can still ionise")
    adaptive = dict(decks.adaptive_time_step(), background_density_SI=1e24)
    refused(adaptive, (0, -1.0, 0), 7, "k_beam_partition")
    # the plasma-plasma setter still takes an adaptive deck, and still refuses species 2 in its own words
    e = api.SliceEngine(adaptive, tile_size=0)
    e.add_collision(0, 0, 5.0, 0)
    with pytest.raises(HpsError, match="species are 0"):
        e.add_collision(0, 2, 5.0, 0)
    # one list for both kinds: 7 + 1 are accepted, a ninth of either kind is not
    for ninth in ("beam", "plasma"):
        e = api.SliceEngine(dense, tile_size=0)
        for _ in range(7):
            e.add_collision(0, 0, 5.0, 0)
        e.add_beam_collision(0, 5.0, 0)
        with pytest.raises(HpsError, match="at most") as err:
            e.add_beam_collision(0, 5.0, 0) if ninth == "beam" else e.add_collision(0, 0, 5.0, 0)
        assert "status 1:" in str(err.value)
    # no beam at all, and a static beam: accepted, nothing collides
    for deck in (dict(dense, beam_profile=-1), dict(dense, dt=0.0)):
        e = api.SliceEngine(dict(deck, collisions=[("beam", 0, 5.0, 3)]), tile_size=16)
        e.run_step()
        assert e.collision_stats() == dict(pairs_collided=0, overfull_cells=0)
    # a deck entry reaches the setter; a mixed list runs in order; a fused schedule is switched off
    e = api.SliceEngine(dict(dense, collisions=[(0, 0, 5.0, 3), ("beam", 0, 5.0, 4)]), tile_size=16)
    e.set_fusion(True)
    e.run_step()
    both = e.collision_stats()["pairs_collided"]
    e = api.SliceEngine(dict(dense, collisions=[(0, 0, 5.0, 3)]), tile_size=16)
    e.run_step()
    assert both > e.collision_stats()["pairs_collided"] > 0


def test_steps_in_flight_hand_on_the_collided_beam(api):
    """three steps of the moving deck: one serial engine against run_local_pipeline with three stages.  Every checksum of every
    step and the beam after the last step (as a set: the partition places particles with atomics) to 1e-10, the bound of the
    serial-against-in-flight tests of tests/test_gpu_parity.py and tests/test_host_beam_gpu.py."""
    import torch
    from hipace_amd.pipeline import run_local_pipeline
    deck = dict(moving_deck(), collisions=[("beam", 0, -1.0, 9)])
    beam = moving_beam(deck)

    def engine():
        e = api.SliceEngine(deck, tile_size=16)
        e.set_beam_particles(beam, allow_outside=True)
        e.set_diagnostics(True)
        return e

    ser = engine()
    want = []
    for _ in range(3):
        ser.run_step()
        want.append(ser.checksums())
    assert ser.collision_stats()["pairs_collided"] > 1000
    bw, sw = ser.beam_state()
    got, beams = {}, {}

    def on_end(step, e):
        e.sync()
        got[step] = e.checksums()
        beams[step] = e.beam_state()
    run_local_pipeline([engine() for _ in range(3)], 3, torch.device("cuda", 0), on_end)
    assert sorted(got) == [0, 1, 2]
    for step in range(3):
        for k, v in want[step].items():
            assert abs(got[step][k] - v) <= 1e-10 * abs(v), (step, k, got[step][k], v)
    bg, sg = beams[2]
    assert np.array_equal(bg, bw)
    worst = 0.0
    for p in range(deck["nz"]):
        a, b = sw[:, bw[p]:bw[p + 1]], sg[:, bg[p]:bg[p + 1]]
        if a.shape[1]:
            worst = max(worst, (np.abs(b[:, match(a[:3], b[:3])] - a).max(axis=1) / np.abs(sw).max(axis=1)).max())
    print(f"beam after three steps, in flight against serial: {worst:.3e}")
    assert worst <= 1e-10
