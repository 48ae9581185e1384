"""The engine's electron push reads validity off psi_half by default (HPS_VALID_BY_PSI, =0: the valid bit of idcpu).

That needs "valid <=> psi_half != 0" on the engine's own electron sheet at every point where the tiled push runs: after every way
a plasma is initialised, after the QSA drop of the depositions and the absorbing boundary of the pushes have invalidated
particles, and for the electrons an ionisable species appends behind the sorted body.  SliceEngine.schedule() says which
variant an engine runs.
"""
import os

import numpy as np
import pytest

from hipace_amd import decks
from hipace_amd._lib import PL_REAL

pytestmark = pytest.mark.gpu

PSI_HALF = PL_REAL.index("psi_half")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def make_engine(api, deck, switch=None, **kw):
    """an engine created with HPS_VALID_BY_PSI = switch (None: not in the environment, the default)"""
    old = os.environ.pop("HPS_VALID_BY_PSI", None)
    if switch is not None:
        os.environ["HPS_VALID_BY_PSI"] = switch
    try:
        return api.SliceEngine(deck, tile_size=16, **kw)
    finally:
        os.environ.pop("HPS_VALID_BY_PSI", None)
        if old is not None:
            os.environ["HPS_VALID_BY_PSI"] = old


def run_slices(eng, deck, n):
    eng.begin_step()
    for k in range(deck["nz"] - 1, deck["nz"] - 1 - n, -1):
        eng.solve_slice(k)
    eng.sync()


def assert_invariant(eng):
    real, valid = eng.particles()
    nz = real[PSI_HALF] != 0.0
    bad = np.flatnonzero(nz != (valid != 0))
    assert bad.size == 0, (bad[:8], real[PSI_HALF][bad[:8]], valid[bad[:8]])
    assert np.all(real[2][valid == 0] == 0.0)       # (and the weight: HPS_VALID_BY_W)
    return int((valid != 0).sum()), int((valid == 0).sum())


def _parsed():
    d = decks.blowout_wake()
    d.update(decks.DENSITY_EXPR_DEFAULT)
    d.update(plasma_density_expr="exp(-(x^2+y^2)/18)", plasma_min_density=0.2)
    return d


def _hollow():
    d = decks.blowout_wake()
    d.update(decks.PLASMA_INIT_DEFAULT)
    d.update(plasma_radius=6.0, plasma_hollow_core_radius=2.0)
    return d


INIT = {
    # name: (deck, invalid slots expected)
    "plain": (decks.blowout_wake, False),
    "parsed_min_density": (_parsed, True),
    "fine_patch": (decks.blowout_wake_fine_patch, False),
    "hollow_core": (_hollow, True),
    "warm_symmetrized": (lambda: decks.blowout_wake_warm(do_symmetrize=True), False),
}


@pytest.mark.parametrize("way", sorted(INIT))
def test_invariant_after_begin_step(api, way):
    make, some_dead = INIT[way]
    deck = make()
    assert deck["nx"] == deck["ny"] == 64
    eng = make_engine(api, deck)
    assert eng.schedule()["valid_by_psi"] is True
    eng.begin_step()
    live, dead = assert_invariant(eng)
    print(f"{way}: {live} valid, {dead} invalid slots")
    assert live > 0 and (dead > 0) == some_dead


def _dying_deck():
    """128 x 128, absorbing walls, 20 slices around the centre of a driver of peak density 600: electrons near the axis are
    kicked beyond max_qsa_weighting_factor = 35 (the QSA drop: 292 of 65 536) and the fastest of the rest reach the walls (4 628
    absorbed).  The density is the largest of a scan at which two runs of ONE schedule still agree to 3e-13 of each field's
    maximum (400: no QSA drop; 500: 24; 700: 5 288 drops and 4e-12 between two runs of one schedule, 800: 2e-10, 1000: 1e-7 --
    every drop removes charge at once, and the order of the depositions' atomics decides the marginal ones' slice)."""
    d = decks.blowout_wake()
    d.update(nx=128, ny=128, nz=20, n_steps=1, lo=(-8.0, -8.0, -1.2), hi=(8.0, 8.0, 1.2), beam_zmin=-1.19, beam_zmax=1.19,
             bc=2, beam_density=600.0, beam_radius=1.2, beam_pos_std=(0.3, 0.3, 1.41), plasma_ppc=(2, 2))
    return d


def _compare(a, b, deck):
    sa, sb = a.slab(), b.slab()
    for c, nm in enumerate(a.comp_names()):
        sc = max(np.abs(sb[c]).max(), 1e-300)
        assert np.abs(sa[c] - sb[c]).max() <= 1e-12 * sc, nm
    (ra, va), (rb, vb) = a.particles(), b.particles()
    assert ra.shape == rb.shape
    assert int(va.sum()) == int(vb.sum()) and np.array_equal(va, vb)      # counts and flags exact


def test_invariant_after_20_slices_with_both_invalidations(api):
    deck = _dying_deck()
    eng = make_engine(api, deck)
    assert eng.schedule()["valid_by_psi"] is True
    eng.begin_step()
    live0, dead0 = assert_invariant(eng)
    assert dead0 == 0
    for k in range(deck["nz"] - 1, -1, -1):
        eng.solve_slice(k)
    eng.sync()
    live, dead = assert_invariant(eng)
    qsa = eng.qsa_drops()
    absorbed = dead - qsa
    print(f"{live} valid, {dead} invalid: {qsa} QSA drops, {absorbed} absorbed at the walls")
    assert live + dead == live0 and qsa > 0 and absorbed > 0


@pytest.mark.parametrize("which", ["plain", "dying"])
def test_default_against_idcpu(api, which):
    deck = decks.blowout_wake() if which == "plain" else _dying_deck()
    n = 20
    on, off = make_engine(api, deck), make_engine(api, deck, "0")
    assert on.schedule()["valid_by_psi"] is True and off.schedule()["valid_by_psi"] is False
    assert make_engine(api, deck, "1").schedule()["valid_by_psi"] is True
    run_slices(on, deck, n)
    run_slices(off, deck, n)
    _compare(on, off, deck)
    if which == "dying":
        assert on.qsa_drops() == off.qsa_drops() > 0


def test_ionisable_species(api):
    """The laser + dopant deck at its test size, ten slices around the pulse's centre: the electrons nitrogen releases are
    appended behind the sorted body with psi_half = 1."""
    deck = decks.laser_ionization_SI()
    kp_inv = 10.0e-6
    deck.update(nx=128, ny=128, nz=10, laser_solver=1, n_steps=1, lo=(deck["lo"][0], deck["lo"][1], -1.125 * kp_inv),
                hi=(deck["hi"][0], deck["hi"][1], 1.125 * kp_inv))
    eng = make_engine(api, deck, sort_period=7)
    on = eng.schedule()["valid_by_psi"]
    run_slices(eng, deck, 10)
    released, _ = eng.ion_stats()
    print(f"valid_by_psi {on}, {released} electrons released")
    assert released > 0
    if on:
        assert_invariant(eng)
