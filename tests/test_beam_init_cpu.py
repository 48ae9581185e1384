"""The general fixed_ppc beam without a GPU: the properties of the numpy restatement the GPU tests compare against
(tests/beam_init_reference.py), the deck's key group, decks.beam_profile_expr against the formula of the engine's host
generator, the refusals Python makes itself, and the exported symbol."""
import ctypes
import os
import re

import numpy as np
import pytest

from hipace_amd import _lib, decks, expr
from hipace_amd import api as A
from tests import beam_init_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_deck(**kw):
    d = decks.blowout_wake()
    d.update(nx=12, ny=9, nz=6, lo=(-3.0, -2.25, -1.5), hi=(3.0, 2.25, 1.5), beam_profile=1, beam_density=2.0, beam_ppc=(2, 1, 3),
             beam_zmin=-1.1, beam_zmax=0.7, beam_radius=1.0e3, beam_pos_mean=(0.0, 0.0, 0.0))
    d.update(kw)
    return d


def const(v):
    return lambda x, y, z: np.full(np.shape(x), float(v))


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ppc", [(1, 1, 1), (2, 2, 1), (2, 1, 3)])
def test_flattop_count_in_closed_form(ppc):
    d = small_deck(beam_ppc=ppc)
    b = R.fixed_ppc_beam(d, const(2.0))
    want = R.flattop_count(d)
    assert want > 0 and b["soa"].shape[1] == want == b["off"][-1]
    # zmin, zmax fall between the sub-positions of a cell for ppc_z = 3: the slices at the ends are partly filled
    per_slice = np.diff(b["off"])
    full = d["nx"] * d["ny"] * int(np.prod(ppc))
    assert per_slice.max() == full and (per_slice[per_slice > 0].min() < full) == (ppc[2] == 3)
    _, _, nppc, scale = R.geometry(d)
    assert np.array_equal(b["soa"][6], np.full(want, abs(2.0 * scale))) and scale == 1.0 / nppc


def test_si_weights_carry_the_cell_volume():
    d = small_deck(si_units=1)
    h, c, nppc, scale = R.geometry(d)
    assert c == 299792458.0 and scale == h[0] * h[1] * h[2] / nppc
    b = R.fixed_ppc_beam(d, const(-3.0), min_density=-np.inf)
    assert np.array_equal(b["soa"][6], np.full(b["soa"].shape[1], abs(-3.0 * scale)))
    assert np.array_equal(b["soa"][5], np.full(b["soa"].shape[1], d["beam_umean"][2] * c))


def test_order_head_first_then_j_i_ipart():
    d = small_deck(beam_radius=1.7, beam_pos_mean=(0.4, -0.3, 0.0))
    b = R.fixed_ppc_beam(d, lambda x, y, z: 1.0 + 0.1 * x)
    off, slot, soa = b["off"], b["slot"], b["soa"]
    h, _, nppc, _ = R.geometry(d)
    assert 0 < soa.shape[1] < d["nx"] * d["ny"] * d["nz"] * nppc
    for p in range(d["nz"]):
        k = d["nz"] - 1 - p
        s = slot[off[p]:off[p + 1]]
        assert (s // (nppc * d["nx"] * d["ny"]) == k).all()                     # block p is slice nz - 1 - p
        assert (np.diff(s) > 0).all()                                             # ((k ny + j) nx + i) nppc + i_part ascends
        z = soa[2, off[p]:off[p + 1]]
        assert ((z >= d["lo"][2] + k * h[2]) & (z < d["lo"][2] + (k + 1) * h[2])).all()
    rx, ry = soa[0] - 0.4, soa[1] + 0.3
    assert (rx * rx + ry * ry <= 1.7 ** 2).all() and (soa[2] >= d["beam_zmin"]).all() and (soa[2] < d["beam_zmax"]).all()


def test_sub_indices_are_those_of_get_position_unit_cell():
    ppc = (2, 3, 4)
    ip = np.arange(24)
    ix, iy, iz = R.unit_cell(ppc, ip)
    assert sorted(zip(ix, iy, iz)) == [(a, b, c) for a in range(2) for b in range(3) for c in range(4)]
    assert (ix[0], iy[1], iz[1], iz[3], ix[12]) == (0, 1, 0, 1, 1)               # y fastest, then z, x slowest


def test_draws_do_not_depend_on_the_evaluation_order():
    d = small_deck(beam_radius=1.6)
    kw = dict(u_std=(0.3, 0.0, 2.0), random_ppc=(1, 1, 0), seed=7)
    whole = R.fixed_ppc_beam(d, const(1.0), **kw)
    off = whole["off"]
    for p in (1, 3):                                                               # a slice on its own: the same particles
        alone = R.fixed_ppc_beam(d, const(1.0), slices=[d["nz"] - 1 - p], **kw)
        assert np.array_equal(alone["soa"], whole["soa"][:, off[p]:off[p + 1]]) and alone["soa"].shape[1] > 0
    perm = np.random.default_rng(0).permutation(whole["slot"].size)
    assert np.array_equal(R.normal_deviates(7, whole["slot"][perm]), whole["normal"][:, perm])
    # position and momentum draws use different keys, another seed other numbers, u_std = 0 draws nothing
    s = whole["slot"][:50]
    assert not np.array_equal(R.uniform_draws(7, R.TAG_POSITION, s, 0), R.uniform_draws(7, R.TAG_MOMENTUM, s, 0))
    assert not np.array_equal(R.uniform_draws(7, R.TAG_POSITION, s, 0), R.uniform_draws(8, R.TAG_POSITION, s, 0))
    assert np.array_equal(whole["soa"][4], np.full(whole["slot"].size, d["beam_umean"][1]))
    u = R.uniform_draws(7, R.TAG_POSITION, whole["slot"], 1)
    assert u.min() >= 0.0 and u.max() < 1.0


def test_random_points_stay_in_their_cells_and_the_corner_is_tested():
    d = small_deck(beam_radius=1.3, beam_ppc=(2, 2, 1))
    h, _, nppc, _ = R.geometry(d)
    b = R.fixed_ppc_beam(d, const(1.0), random_ppc=(1, 1, 0), seed=3)
    soa, slot = b["soa"], b["slot"]
    i, j = (slot // nppc) % d["nx"], (slot // (nppc * d["nx"])) % d["ny"]
    xc, yc = d["lo"][0] + i * h[0], d["lo"][1] + j * h[1]
    assert ((soa[0] >= xc) & (soa[0] < xc + h[0]) & (soa[1] >= yc) & (soa[1] < yc + h[1])).all()
    assert (xc * xc + yc * yc <= 1.3 ** 2).all()                                    # every cell corner inside the radius ...
    assert (soa[0] ** 2 + soa[1] ** 2 > 1.3 ** 2).any()                             # ... some particles beyond it
    assert (np.unique(slot // nppc, return_counts=True)[1] == nppc).all()            # a cell is taken whole
    k = slot // (nppc * d["nx"] * d["ny"])
    assert np.array_equal(soa[2], d["lo"][2] + (k + 0.5) * h[2])


def test_min_density_drops_the_point_that_equals_it():
    d = small_deck(beam_ppc=(1, 1, 1))
    x0 = d["lo"][0] + 2.5 * R.geometry(d)[0][0]                                     # a lattice position
    f = lambda x, y, z: np.where(x == x0, 0.25, 1.0)      # noqa: E731
    a = R.fixed_ppc_beam(d, f, min_density=0.25)
    b = R.fixed_ppc_beam(d, f, min_density=0.2499)
    assert not (a["soa"][0] == x0).any() and (b["soa"][0] == x0).any() and a["soa"].shape[1] < b["soa"].shape[1]


# ---- the deck ---------------------------------------------------------------------------------------------------------------

def test_key_group_is_kept_apart_from_the_default_deck():
    assert decks.BEAM_INIT_DEFAULT == dict(beam_density_expr=None, beam_min_density=0.0, beam_u_std=(0, 0, 0), beam_random_ppc=(0, 0, 0),
                                           beam_seed=1, beam_density_constants=None)
    assert not set(decks.BEAM_INIT_DEFAULT) & set(decks._DEFAULT)
    assert not set(decks.BEAM_INIT_DEFAULT) & {n for n, _ in _lib.Deck._fields_}
    for make in (decks.blowout_wake, decks.linear_wake, decks.beam_evolution, decks.adaptive_time_step, decks.blowout_wake_warm):
        assert not set(decks.BEAM_INIT_DEFAULT) & set(make())
        assert decks.beam_init(make()) is None                                      # no call for a deck without the keys
    assert decks.beam_init(dict(decks.blowout_wake(), **decks.BEAM_INIT_DEFAULT)) is None


def test_hollow_beam_deck_is_the_blowout_deck_with_a_ring():
    d, base = decks.blowout_wake_hollow_beam(), decks.blowout_wake()
    assert set(d) - set(base) == set(decks.BEAM_INIT_DEFAULT)
    assert {k for k in base if base[k] != d[k]} == set()
    spec = decks.beam_init(d)
    assert spec["min_density"] == 0.0 and spec["u_std"] == (0.0, 0.0, 0.0) and spec["random_ppc"] == (0, 0, 0) and spec["seed"] == 1
    p = expr.compile_expr(spec["expr"], ("x", "y", "z"), spec["constants"])
    r = np.array([0.0, 0.59, 0.6, 0.99, 1.0])
    v = p.evaluate(r, 0.0 * r, 0.0 * r)
    assert list(v) == [0.0, 0.0, 1.0, 1.0, 0.0]
    assert p.evaluate(0.8, 0.0, 1.41) == np.exp(-0.5 * (1.41 / 1.41) ** 2)
    assert d["beam_radius"] >= 1.0
    import pickle
    assert pickle.loads(pickle.dumps(d)) == d


@pytest.mark.parametrize("profile", [0, 1])
def test_beam_profile_expr_is_the_host_generators_formula(profile):
    d = dict(decks.blowout_wake(), beam_profile=profile, beam_pos_mean=(0.3, -0.2, 0.1), beam_pos_std=(0.4, 0.5, 1.3), beam_density=2.5)
    text, consts = decks.beam_profile_expr(d)
    p = expr.compile_expr(text, ("x", "y", "z"), consts)
    rng = np.random.default_rng(5)
    x, y, z = rng.uniform(-3, 3, (3, 4000))
    got = p.evaluate(x, y, z)
    if profile == 1:
        assert np.array_equal(got, np.full(x.shape, 2.5))
        return
    # Engine::init_beam's beam_density_at, operation by operation
    a, b, c = (x - 0.3) / 0.4, (y + 0.2) / 0.5, (z - 0.1) / 1.3
    want = 2.5 * np.exp(-0.5 * a * a) * np.exp(-0.5 * b * b) * np.exp(-0.5 * c * c)
    assert np.array_equal(got, want) and want.min() > 0.0


def test_python_refusals():
    base = decks.blowout_wake()
    for bad in (dict(beam_min_density=0.1), dict(beam_u_std=(0.0, 0.0, 1.0)), dict(beam_random_ppc=(1, 0, 0))):
        with pytest.raises(ValueError, match="beam_profile_expr"):
            decks.beam_init(dict(base, **bad))
    with pytest.raises(ValueError, match="no beam profile"):
        decks.beam_profile_expr(dict(base, beam_profile=-1))
    # an expression that reads t: refused before the library is called (no engine behind this object)
    eng = object.__new__(A.SliceEngine)
    eng._h = None
    for bad in ("x*t", expr.compile_expr("x + t")):
        with pytest.raises(ValueError, match="cannot read t"):
            eng.set_beam_fixed_ppc(bad)
    with pytest.raises(ValueError, match="unknown name"):
        eng.set_beam_fixed_ppc("x*q")


def test_adaptive_initial_estimate_takes_the_beams_u_std():
    d = dict(decks.adaptive_time_step(), **decks.BEAM_INIT_DEFAULT)
    d.update(beam_density_expr="1", beam_u_std=(0.0, 0.0, 10.0))
    want = A.AdaptiveTimeStep(dict(decks.adaptive_time_step(), beam_uz_std=10.0)).initial_dt()
    assert A.AdaptiveTimeStep(d).initial_dt() == want != A.AdaptiveTimeStep(decks.adaptive_time_step()).initial_dt()
    # the deck's own beam_uz_std wins
    assert A.AdaptiveTimeStep(dict(d, beam_uz_std=5.0)).initial_dt() == A.AdaptiveTimeStep(dict(decks.adaptive_time_step(), beam_uz_std=5.0)).initial_dt()


# ---- the library ------------------------------------------------------------------------------------------------------------

def test_symbol_header_and_binding():
    _lib.build()
    L = ctypes.CDLL(_lib.SO)
    assert hasattr(L, "hps_engine_set_beam_fixed_ppc")
    hdr = open(os.path.join(ROOT, "include", "hpslice.h")).read()
    assert re.search(r"\bint\s+hps_engine_set_beam_fixed_ppc\s*\(", hdr)
    assert len(_lib._SIGS["hps_engine_set_beam_fixed_ppc"][1]) == 6
    assert "beam_init.hip" in open(os.path.join(ROOT, "hipace_amd", "csrc", "Makefile")).read()
