"""Binary Coulomb collisions on the GPU: the operator against the numpy restatement particle by particle, order
independence, conservation, the engine's placement and keys, the refusals, and the reference's checksum file."""
import json
import os

import numpy as np
import pytest

from hipace_amd import decks
from tests import collision_reference as R
from tests.collision_util import deviation, from_gpu, geometry, sheet_arrays, sheet_from, small_deck, to_gpu, write_thermal
from tests.test_collisions_cpu import CONSERVATION_BOUND, conservation_cases, conservation_error

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# Largest |u_gpu - u_numpy| / rms(u of the cell) over every particle of every operator case below, measured on the MI355X:
# 3.8e-14 (case same_si_auto_all_branches; device log / exp / sinh / cos / cbrt against numpy's).  Asserted: ten times that,
# far below the 1e-9 that tests/test_gpu_parity.py gives operators with transcendental functions.
OPERATOR_BOUND = 3.8e-13
BIG_CELL = 27


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()
    return A


# name: (si, two species, kwargs of thermal_cells for species a, weight scale, coulomb_log, background density, tail, expected branches)
CASES = {
    "same_norm_auto": dict(si=False, L=-1.0, bg=1.0e24),
    "same_norm_fixed_dense": dict(si=False, L=10.0, bg=1.0e30),
    "same_si_auto": dict(si=True, L=-1.0, wscale=1.0e8),
    "same_si_fixed_all_branches": dict(si=True, L=10.0, wscale=1.0e10, branches=(0, 1, 2, 3)),
    "same_si_auto_all_branches": dict(si=True, L=-1.0, wscale=1.0e10, branches=(0, 1, 2, 3)),
    "two_species_norm": dict(si=False, L=-1.0, bg=1.0e28, two=True),
    "two_species_si_ionisable": dict(si=True, L=10.0, wscale=1.0e9, two=True, levels=True),
    "same_norm_ionisable": dict(si=False, L=-1.0, bg=1.0e26, levels=True),
    "same_norm_invalid_and_outside": dict(si=False, L=-1.0, bg=1.0e24, spoil=True),
}
_reference = {}


def reference_case(name):
    """(sheet a before, sheet b before or None, a after, b after, log, lo, dx), computed once per session"""
    if name in _reference:
        return _reference[name]
    k = CASES[name]
    si = k["si"]
    a, lo, dx = R.thermal_cells(21, si=si, big_cell=BIG_CELL, mixed_levels=k.get("levels", False))
    a["w"] *= k.get("wscale", 1.0)
    b = None
    if k.get("two"):
        b, _, _ = R.thermal_cells(22, si=si, scale=2.0, u_std=0.002, key_offset=7)      # other counts per cell, colder and heavier
        b["w"] *= k.get("wscale", 1.0)
    if k.get("spoil"):
        a["valid"][::7] = 0
        a["w"][3::11] = 0.0
        a["x"][5::13] = lo[0] + (R.NX + 0.5) * dx
    a0, b0 = R.copy_sheet(a), (R.copy_sheet(b) if b is not None else None)
    q, m = (-R.QE, R.ME) if si else (-1.0, 1.0)
    log = R.collide(a, b if b is not None else a, R.NX, R.NY, lo, dx, dx, dx, q, m, -q, 1836.0 * m, can_ionize_a=k.get("levels", False),
                    coulomb_log=k["L"], background_density_SI=k.get("bg", 0.0), normalized=not si, seed=77, collision=1, step=3, islice=5)
    _reference[name] = (a0, b0, a, b, log, lo, dx)
    return _reference[name]


def run_gpu(api, name, a0, b0, lo, dx, tiling=None):
    k = CASES[name]
    si = k["si"]
    q, m = (-R.QE, R.ME) if si else (-1.0, 1.0)
    ga = to_gpu(api, a0)
    gb = to_gpu(api, b0) if b0 is not None else ga
    pairs, over = api.CoulombCollision(ga, gb, geometry(api, lo, dx, si), q, m, -q, 1836.0 * m, can_ionize_a=k.get("levels", False),
                                       coulomb_log=k["L"], background_density_SI=k.get("bg", 0.0), seed=77, collision=1, step=3, islice=5)
    return from_gpu(ga), (from_gpu(gb) if b0 is not None else None), pairs, over


@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_matches_the_numpy_restatement(api, name):
    a0, b0, a, b, log, lo, dx = reference_case(name)
    k = CASES[name]
    for br in k.get("branches", ()):
        assert log["branch"][br] > 0, (name, log["branch"])
    if not k.get("levels") and not k.get("two"):
        assert log["rejected"][0] > 0 and log["rejected"][1] > 0      # unequal weights: both rejection draws decide
    ua, ub, pairs, over = run_gpu(api, name, a0, b0, lo, dx)
    c = R.C_SI if k["si"] else 1.0
    dev = deviation(a, ua, c, lo, dx)
    if b is not None:
        dev = max(dev, deviation(b, ub, c, lo, dx))
    print(f"{name}: deviation {dev:.3e} pairs {pairs} (numpy {log['pairs']}) overfull {over} branches {log['branch']}")
    assert pairs == log["pairs"]
    assert over >= 1                      # the cell of 1500 does not fit the LDS stage
    assert dev <= OPERATOR_BOUND, (name, dev)


def test_union_of_cases_reaches_every_branch_of_the_sampler():
    seen = np.zeros(4, dtype=int)
    for name in CASES:
        seen += np.array(reference_case(name)[4]["branch"])
    assert (seen > 0).all(), seen


def test_result_does_not_depend_on_sheet_order_or_tiling(api):
    name = "two_species_norm"
    a0, b0, _, _, _, lo, dx = reference_case(name)
    ua, ub, _, _ = run_gpu(api, name, a0, b0, lo, dx)
    rng = np.random.default_rng(1)
    pa, pb = rng.permutation(len(a0["x"])), rng.permutation(len(b0["x"]))
    sa, sb = {k: v[pa] for k, v in a0.items()}, {k: v[pb] for k, v in b0.items()}
    va, vb, _, _ = run_gpu(api, name, sa, sb, lo, dx)
    for q in range(3):
        assert np.array_equal(ua[q][pa], va[q]) and np.array_equal(ub[q][pb], vb[q])
    # the same sheet passed through the 16- and 32-cell tile sorts (invalid particles last), and with a tail of particles
    # behind the tile-sorted body; the shuffled order above is the stronger half of this test on an 8 x 8 grid
    geom = geometry(api, lo, dx, False)
    for ts, tail in ((16, 0), (32, 0), (16, 200)):
        n = len(a0["x"]) - tail
        body = {k: v[:n] for k, v in a0.items()}
        g_body = to_gpu(api, body)
        tiling = api.Tiling(R.NX, R.NY, ts, n)
        g_sorted = tiling.reorder(g_body, geom)
        real, _ = g_sorted.numpy()
        idc = g_sorted.idcpu.cpu().numpy().view(np.uint64)
        key = ((idc >> np.uint64(24)) & np.uint64((1 << 39) - 1)).astype(np.int64) - 1
        by_key = {int(kk): i for i, kk in enumerate(a0["key"])}
        order = np.array([by_key[int(kk)] for kk in key] + list(range(n, n + tail)), dtype=np.int64)
        assert sorted(order.tolist()) == list(range(len(a0["x"])))
        ta = {k: v[order] for k, v in a0.items()}
        wa, wb, _, _ = run_gpu(api, name, ta, b0, lo, dx)
        for q in range(3):
            assert np.array_equal(ua[q][order], wa[q]) and np.array_equal(ub[q], wb[q]), (ts, tail, q)


def test_gpu_conserves_momentum_and_energy_per_cell(api):
    for name, s, lo, dx, si, kw in conservation_cases():
        q, m = (-R.QE, R.ME) if si else (-1.0, 1.0)
        g = to_gpu(api, s)
        pairs, _ = api.CoulombCollision(g, g, geometry(api, lo, dx, si), q, m, coulomb_log=kw["coulomb_log"],
                                        background_density_SI=0.0 if si else 1.0e24, seed=kw["seed"])
        after = R.copy_sheet(s)
        after["ux"], after["uy"], after["psi"] = from_gpu(g)
        ep, ee = conservation_error(s, after, m, R.C_SI if si else 1.0, lo, dx)
        print(f"{name}: pairs {pairs} momentum {ep:.3e} energy {ee:.3e}")
        assert pairs > 300 and ep <= CONSERVATION_BOUND and ee <= CONSERVATION_BOUND, (name, ep, ee)


# ---- the engine --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(0, 0), (0, 1)])
def test_engine_collides_behind_the_push_with_the_slice_key(api, pair):
    from hipace_amd import _lib
    L = _lib.lib()
    if pair == (0, 0):
        deck = small_deck(decks.blowout_wake(), background_density_SI=1.0e24)
    else:
        deck = small_deck(decks.ion_motion_SI(), ion_ppc=(2, 2))
    si = bool(deck["si_units"])
    u_std = 0.05 * (R.C_SI if si else 1.0)
    engines = []
    for collide in (True, False):
        e = api.SliceEngine(deck, tile_size=0)
        if collide:
            e.add_collision(pair[0], pair[1], -1.0, 42)
        e.begin_step()
        e.sync()
        write_thermal(L.hps_engine_plasma(e._h), 1, u_std)
        if pair[1] == 1:
            write_thermal(L.hps_engine_ions(e._h), 2, u_std / 50.0)
        e.solve_slice(deck["nz"] - 1)
        e.sync()
        engines.append(e)
    with_c, without = engines
    assert with_c.collision_stats()["pairs_collided"] > 1000
    el_c, id_c, lev_c = sheet_arrays(api, L.hps_engine_plasma(with_c._h))
    el_p, _, _ = sheet_arrays(api, L.hps_engine_plasma(without._h))
    assert np.abs(el_c[8:] - el_p[8:]).max() > 1e-6 * u_std          # the collision did something
    # tile size 0 keeps the lattice order: the colliding engine's keys are the plain engine's particle indices
    assert np.array_equal((id_c >> np.uint64(24)) & np.uint64((1 << 39) - 1), np.arange(1, len(id_c) + 1, dtype=np.uint64))
    geom = api.Geometry(deck["nx"], deck["ny"], deck["lo"][:2], deck["hi"][:2], (deck["hi"][2] - deck["lo"][2]) / deck["nz"], bc=deck["bc"],
                        normalized=not si, consts=(R.C_SI, R.EP0, 4.0e-7 * np.pi, R.QE, R.ME) if si else (1.0,) * 5)
    sa = sheet_from(api, el_p, id_c, lev_c)
    if pair[1] == 1:
        ion_c, iid_c, ilev_c = sheet_arrays(api, L.hps_engine_ions(with_c._h))
        ion_p, _, ilev_p = sheet_arrays(api, L.hps_engine_ions(without._h))
        sb = sheet_from(api, ion_p, iid_c, ilev_p)
        api.CoulombCollision(sa, sb, geom, deck["plasma_charge"], deck["plasma_mass"], deck["ion_charge"], deck["ion_mass"], can_ionize_b=True,
                             coulomb_log=-1.0, background_density_SI=deck["background_density_SI"], seed=42, collision=0, step=0,
                             islice=deck["nz"] - 1)
        got_b = from_gpu(sb)
    else:
        api.CoulombCollision(sa, sa, geom, deck["plasma_charge"], deck["plasma_mass"], coulomb_log=-1.0,
                             background_density_SI=deck["background_density_SI"], seed=42, collision=0, step=0, islice=deck["nz"] - 1)
    got = from_gpu(sa)
    c = R.C_SI if si else 1.0
    scale = np.array([u_std, u_std, 0.05])[:, None]
    dev = (np.abs(np.stack(got) - el_c[8:]) / scale).max()
    if pair[1] == 1:
        dev = max(dev, (np.abs(np.stack(got_b) - ion_c[8:]) / (scale / 50.0)).max())
    print(f"pair {pair}: engine against operator {dev:.3e} (c = {c})")
    assert dev <= OPERATOR_BOUND


def _head_slice_state(api, deck, collide):
    e = api.SliceEngine(deck, tile_size=0)
    if collide:
        e.add_collision(0, 0, -1.0, 1)
    e.set_diagnostics(True)
    e.begin_step()
    e.solve_slice(deck["nz"] - 1)
    real, _ = e.particles()
    return real, e.slab(), e.checksums(), (e.collision_stats() if collide else None)


def test_engine_without_pairs_is_the_engine_without_collisions(api):
    """A cold 1 x 1 ppc plasma holds one particle per cell when the head slice's collisions run: no pair, no change.  The
    per-particle deposition adds with atomics in no fixed order, so two plain runs are compared first: where they agree bit
    for bit the run with a collision must too; otherwise the engine-against-engine bound of tests/test_gpu_parity.py (1e-9 of
    the largest entry) is asserted instead."""
    deck = dict(decks.blowout_wake(), n_steps=1, background_density_SI=1.0e24)
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


def test_refusals(api):
    from hipace_amd._lib import HpsError
    def refused(deck, args, status, text, begin=False):
        e = api.SliceEngine(deck, tile_size=0)
        if begin:
            e.begin_step()
        with pytest.raises(HpsError) as err:
            e.add_collision(*args)
        assert f"status {status}:" in str(err.value) and text in str(err.value), str(err.value)
    small = small_deck(decks.blowout_wake())
    refused(small, (0, 0, -1.0, 0), 1, "background_density_SI")
    refused(dict(small, background_density_SI=1e24), (0, 1, -1.0, 0), 1, "ion_on")
    refused(dict(small, background_density_SI=1e24), (0, 2, -1.0, 0), 1, "species are 0")
    refused(dict(small, background_density_SI=1e24), (0, 0, -1.0, 0), 1, "before the first hps_engine_begin_step", begin=True)
    refused(small_deck(decks.ionization_SI(), plasma_ppc=(0, 0)), (0, 1, -1.0, 0), 7, "can still ionise")
    e = api.SliceEngine(dict(small, background_density_SI=1e24), tile_size=0)
    for _ in range(8):
        e.add_collision(0, 0, 5.0, 0)
    with pytest.raises(HpsError, match="at most"):
        e.add_collision(0, 0, 5.0, 0)
    # a deck entry reaches the setter, and a fused schedule is switched off rather than deposited ahead of the collisions
    e = api.SliceEngine(dict(small, background_density_SI=1e24, collisions=[(0, 0, 5.0, 3)]), tile_size=16)
    e.set_fusion(True)
    e.run_step()
    assert e.collision_stats()["pairs_collided"] > 0


def test_collisions_SI_fixture(api):
    """tests/collisions.SI.1Rank.sh against the reference's checksum file.  A WEAK, statistical pin: the reference draws from
    amrex::Random, a different stream, and at 1 x 1 ppc only the bunched sheath cells hold pairs.  Per field the deviation of
    the seed-0 run from the file must stay within three times the spread (max - min) of the engine's own checksums over five
    seeds, plus the 1e-9 of the value that the fixtures without random draws are held to."""
    gold = json.load(open(os.path.join(GOLD, "collisions.SI.1Rank.json")))
    def run(deck):
        e = api.SliceEngine(deck, tile_size=0)
        e.set_diagnostics(True)
        e.run_step()
        return e, e.checksums()
    runs = [run(dict(decks.collisions_SI(seed=s), n_steps=1)) for s in range(5)]
    _, plain = run(dict(decks.blowout_wake_SI(), n_steps=1))
    assert runs[0][0].collision_stats()["pairs_collided"] > 0
    bad = []
    for k, v in gold["lev=0"].items():
        vals = [cs[k] for _, cs in runs]
        spread = max(vals) - min(vals)
        dev, dev_plain = abs(vals[0] - v), abs(plain[k] - v)
        print(f"{k}: file {v:.10e} spread/|v| {spread / max(abs(v), 1e-300):.2e} deviation/|v| {dev / max(abs(v), 1e-300):.2e} "
              f"without collisions {dev_plain / max(abs(v), 1e-300):.2e}")
        if dev > 3.0 * spread + 1e-9 * abs(v):
            bad.append(k)
    # the beam is static (hipace.dt = 0): its checksums are the injected beam's
    _, soa = runs[0][0].beam_state()
    gb = gold["beam"]
    mine = dict(x=np.abs(soa[0]).sum(), y=np.abs(soa[1]).sum(), z=np.abs(soa[2]).sum(), uz=np.abs(soa[5]).sum() / R.C_SI, w=np.abs(soa[6]).sum())
    for k, v in mine.items():
        print(f"beam {k}: {v:.10e} file {gb[k]:.10e}")
        if abs(v - gb[k]) > 1e-9 * abs(gb[k]):
            bad.append("beam " + k)
    assert not bad, bad
