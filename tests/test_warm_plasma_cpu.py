"""Warm plasmas without a GPU: the numpy restatement of the momentum draws, the mirror copies and the shifted lattice
(tests/plasma_thermal_reference.py) against their defining properties, and the host layer (deck keys, the temperature
conversion, the exported symbols).  The engine's sheets are compared with the restatement in tests/test_warm_plasma_gpu.py."""
import ctypes

import numpy as np
import pytest

from hipace_amd import decks
from tests import plasma_init_reference as R
from tests import plasma_thermal_reference as W

SEED = 1                       # the seed of the GPU tests too
N = 16384
LO, HI = (-8.0, -8.0, -6.0), (8.0, 8.0, 6.0)


def corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def test_draw_statistics():
    """Conditions on fixed inputs (seed 1, slots 0 .. 16383, species 0, steps 0 and 1).  Observed, in units of the bound / 5:
    means 0.57 0.44 -0.74 (of u_std / sqrt N), variances 0.13 -0.59 0.14 (of sqrt(2 / N)), correlations between components
    0.82 -1.67 -1.02, between slots k and k + 1 1.21 0.30 -1.04, between steps 0 and 1 0.47 1.92 0.92 (of 1 / sqrt N)."""
    u_std = (0.3, 0.02, 1.5)
    slots = np.arange(N)
    n0, n1 = W.normal_deviates(SEED, 0, 0, slots), W.normal_deviates(SEED, 0, 1, slots)
    assert np.isfinite(n0).all() and np.isfinite(n1).all()
    u, ux, uy, psi = W.momenta(slots, (0.0, 0.0, 0.0), u_std, SEED, 0, 0)
    assert np.isfinite(u).all() and np.isfinite(psi).all() and psi.min() > 0.0
    for d in range(3):
        assert abs(u[d].mean()) <= 5.0 * u_std[d] / np.sqrt(N), d
        assert abs(u[d].var() / u_std[d] ** 2 - 1.0) <= 5.0 * np.sqrt(2.0 / N), d
    bound = 5.0 / np.sqrt(N)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs(corr(n0[a], n0[b])) <= bound, (a, b)
    for d in range(3):
        assert abs(corr(n0[d][:-1], n0[d][1:])) <= bound, d
        assert abs(corr(n0[d], n1[d])) <= bound, d
    # the species is a link of the chain too
    assert abs(corr(n0[0], W.normal_deviates(SEED, 1, 0, slots)[0])) <= bound


def test_hash_chain_is_the_uint64_arithmetic():
    """coll_hash with Python integers mod 2^64, link by link"""
    M = (1 << 64) - 1

    def h(x, v):
        z = (x + 0x9E3779B97F4A7C15 * (v + 1)) & M
        for _ in range(2):
            z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M
            z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M
            z ^= z >> 31
        return z

    for seed, species, step, slot, draw in ((0, 0, 0, 0, 0), (1, 1, 3, 4095, 2), (2 ** 64 - 1, 0, 7, 2 ** 27, 3)):
        want = h(h(h(h(seed, species), step), slot), draw)
        got = W.coll_hash(W.slot_key(seed, species, step, np.array([slot], dtype=np.uint64)), np.uint64(draw))[0]
        assert int(got) == want
        assert float(W.coll_unit(got)) == (want >> 11) / 2.0 ** 53
    # u1 = 1 - unit is never 0: the largest unit is 1 - 2^-53
    assert 1.0 - float(W.coll_unit(np.uint64(M))) > 0.0


def test_a_component_without_spread_is_exactly_its_mean():
    u, ux, uy, psi = W.momenta(np.arange(100), (0.1, -0.2, 0.3), (0.0, 0.05, 0.0), SEED, 0, 0, c=2.0)
    assert np.all(u[0] == 0.1) and np.all(u[2] == 0.3) and np.ptp(u[1]) > 0.0
    assert np.array_equal(ux, u[0] * 2.0)
    assert np.array_equal(psi, np.sqrt(1.0 + u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - u[2])


def test_mirror_copies():
    kw = dict(nx=64, ny=64, lo=LO, hi=HI, nz=100, ppc=(1, 1), fine_ppc=(2, 2), T=2, radius=6.0, u_mean=(0.01, 0.0, 0.0),
              u_std=(0.1, 0.2, 0.3), seed=SEED)
    c = -8.0 + (np.arange(64) + 0.5) * 0.25
    mask = np.hypot(c[None, :], c[:, None]) < 2.0
    plain = W.init_particles_warm(mask=mask, **kw)
    sym = W.init_particles_warm(mask=mask, do_symmetrize=True, **kw)
    n = plain["x"].size
    assert sym["x"].size == 4 * n and sym["nslots"] == 4 * plain["nslots"] and sym["nprimary"] == n
    sx, sy = (1, -1, 1, -1), (1, 1, -1, -1)
    for m in range(4):
        s = slice(m * n, (m + 1) * n)
        assert np.array_equal(sym["x"][s], plain["x"] if sx[m] > 0 else 0.0 - plain["x"])
        assert np.array_equal(sym["y"][s], plain["y"] if sy[m] > 0 else 0.0 - plain["y"])
        assert np.array_equal(sym["ux"][s], sx[m] * plain["ux"]) and np.array_equal(sym["uy"][s], sy[m] * plain["uy"])
        assert np.array_equal(sym["psi"][s], plain["psi"])
        assert np.array_equal(sym["w"][s], sym["w"][:n]) and np.array_equal(sym["w"][s], plain["w"] / 4.0)
        assert np.array_equal(sym["slot"][s], plain["slot"] + m * plain["nslots"])
    assert abs(sym["w"].sum() / plain["w"].sum() - 1.0) <= 1e-14
    # an off-centre box mirrors about lo + hi
    off = W.init_particles_warm(32, 32, (-3.0, -1.0, 0.0), (5.0, 7.0, 1.0), 1, (1, 1), do_symmetrize=True)
    q = off["x"].size // 4
    assert np.array_equal(off["x"][q:2 * q], 2.0 - off["x"][:q]) and np.array_equal(off["y"][2 * q:3 * q], 6.0 - off["y"][:q])


def test_slots_are_the_engines_order():
    """slot_of: the reference's order (i_part outermost, x fastest, only those created) is the ascending order of the slots"""
    c = -8.0 + (np.arange(64) + 0.5) * 0.25
    mask = np.hypot(c[None, :], c[:, None]) < 2.0
    p = W.init_particles_warm(64, 64, LO, HI, 100, (1, 1), (4, 4), mask, 2, radius=5.0, hollow_core_radius=1.0)
    assert np.all(np.diff(p["slot"]) > 0) and p["slot"].max() < p["nslots"]
    assert p["nslots"] == 64 * 64 + 15 * int((R.init_particles(64, 64, LO, HI, 100, (1, 1), (4, 4), mask, 2)["L"] > 0).sum())


def lattice(nx, ny, ppc, prevent):
    lo, hi = (-8.0, -8.0, -6.0), (8.0, 8.0, 6.0)
    return W.init_particles_warm(nx, ny, lo, hi, 100, ppc, prevent_centered_particle=prevent)


def test_prevent_centered_particle():
    plain, moved = lattice(63, 63, (1, 1), False), lattice(63, 63, (1, 1), True)
    assert np.any((plain["x"] == 0.0) & (plain["y"] == 0.0))            # the particle the key is there for
    assert not np.any((moved["x"] == 0.0) & (moved["y"] == 0.0))
    assert np.abs(moved["x"]).min() > 0.1 and np.abs(moved["y"]).min() > 0.1
    assert moved["x"].size == 62 * 62 and moved["nslots"] == 63 * 63
    dx = 16.0 / 63
    assert np.array_equal(moved["x"][:62], -8.0 + (np.arange(1, 63) + 0.5 - 0.5) * dx)      # the nodes 1 .. n - 1
    assert np.array_equal(moved["slot"][:62], np.arange(1, 63) + 63)                        # row 0 and column 0 own no particle
    # the shifted lattice is its own mirror image
    assert np.allclose(np.sort(moved["x"]), np.sort(-moved["x"]), rtol=0.0, atol=1e-13)
    # 63 x 64: x only
    a, b = lattice(63, 64, (1, 1), True), lattice(63, 64, (1, 1), False)
    assert a["x"].size == 62 * 64 and np.array_equal(np.unique(a["y"]), np.unique(b["y"])) and not np.any(a["x"] == 0.0)
    a = lattice(64, 63, (1, 1), True)
    assert a["x"].size == 64 * 62 and not np.any(a["y"] == 0.0)
    # ppc 3 x 1 on 63 x 63: both directions, (nx - 1) (ny - 1) cells of 3
    a = lattice(63, 63, (3, 1), True)
    assert a["x"].size == 3 * 62 * 62 and a["nslots"] == 3 * 63 * 63
    # an even ppc or an even grid: nothing moves, bit for bit
    for nx, ny, ppc in ((63, 63, (2, 2)), (64, 64, (1, 1)), (64, 64, (3, 3))):
        a, b = lattice(nx, ny, ppc, True), lattice(nx, ny, ppc, False)
        ref = R.init_particles(nx, ny, (-8.0, -8.0, -6.0), (8.0, 8.0, 6.0), 100, ppc)
        for k in ("x", "y", "w"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], ref[k])
        assert a["x"].size == ppc[0] * ppc[1] * nx * ny
    # mixed: ppc (1, 2) on 63 x 63 shifts x only
    a = lattice(63, 63, (1, 2), True)
    assert a["x"].size == 2 * 62 * 63


def test_shifted_lattice_without_a_shift_is_the_plain_lattice():
    a = W.shifted_lattice(40, 24, LO, HI, 10, (2, 1), (False, False), radius=5.0, hollow_core_radius=1.0, normalized=False)
    b = R.init_particles(40, 24, LO, HI, 10, (2, 1), radius=5.0, hollow_core_radius=1.0, normalized=False)
    for k in ("x", "y", "w", "i", "j", "i_part"):
        assert np.array_equal(a[k], b[k]), k


# ---- host layer -----------------------------------------------------------------------------------------------------------------

def test_temperature_conversion():
    q_e, m_e, c = 1.602176634e-19, 9.1093837015e-31, 299792458.0
    d = decks.blowout_wake_warm(temperature_in_ev=50.0)
    want = np.sqrt(50.0 * q_e / (m_e * c * c))
    assert decks.thermal_u_std(d, "plasma") == pytest.approx((want,) * 3, rel=1e-15)
    assert want == pytest.approx(np.sqrt(50.0 / 510998.95), rel=1e-8)             # kT / (m_e c^2)
    assert d["plasmas_do_symmetrize"] == 1 and d["plasma_u_std"] is None and set(decks.PLASMA_THERMAL_DEFAULT) <= set(d)
    # the species' own mass, in both unit systems
    ion = decks.with_ion_species(dict(d, background_density_SI=1.0e24, ion_temperature_in_ev=3.0), "He", 1.0)
    m_he = 1.67262192369e-27 * 4.002602 / decks.M_P_DA
    assert decks.thermal_u_std(ion, "ion") == pytest.approx((np.sqrt(3.0 * q_e / (m_he * c * c)),) * 3, rel=1e-14)
    si = decks.blowout_wake_SI()
    si.update(decks.PLASMA_THERMAL_DEFAULT)
    si.update(plasma_temperature_in_ev=50.0)
    assert decks.thermal_u_std(si, "plasma") == pytest.approx((want,) * 3, rel=1e-15)
    si_ion = decks.with_ion_species(dict(si, ion_temperature_in_ev=3.0), "He", 1.0e23)
    assert decks.thermal_u_std(si_ion, "ion") == pytest.approx(decks.thermal_u_std(ion, "ion"), rel=1e-14)
    # u_std passes through, nothing given is cold
    assert decks.thermal_u_std(dict(d, plasma_temperature_in_ev=None, plasma_u_std=(0.1, 0.2, 0.3)), "plasma") == (0.1, 0.2, 0.3)
    assert decks.thermal_u_std(decks.blowout_wake(), "plasma") == (0.0, 0.0, 0.0)


def test_u_std_and_a_temperature_exclude_each_other():
    d = decks.blowout_wake_warm()
    with pytest.raises(ValueError, match="exclusively"):
        decks.thermal_u_std(dict(d, plasma_u_std=(0.1, 0.1, 0.1)), "plasma")
    with pytest.raises(ValueError, match="exclusively"):
        decks.thermal_u_std(dict(d, ion_u_std=(0.0, 0.0, 0.0), ion_temperature_in_ev=1.0, ion_mass=1836.0), "ion")


def test_library_exports_the_warm_plasma_setters():
    from hipace_amd import _lib
    _lib.build()
    L = ctypes.CDLL(_lib.SO)
    for name in ("hps_engine_set_plasma_momentum", "hps_engine_set_plasma_symmetry"):
        assert hasattr(L, name), name
        assert name in _lib._SIGS
