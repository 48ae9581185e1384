"""HPS_EARLY_INIT: on the plain explicit-solver slice the shift of the slab and the next slice's zeroing ride as guest
workgroups in the launch of the Bx/By solve's first lower V (k_lower_v3) and write the zeros to alternate planes; observers
(slab(), particles(), sync()) see the slab as without it.  Every comparison is the one of
test_schedules_do_not_change_results (tests/test_gpu_parity.py): each slab component to 1e-12 x max|component|, the particles
to 1e-12, equal sets of valid bits -- two runs of one schedule differ only by the order of their LDS atomics."""
import os

import numpy as np
import pytest

from hipace_amd import decks

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def _deck(nx=128, ny=128, short=False, **kw):
    """blowout_wake on nx x ny cells.  short: the 40 slices around the beam's centre instead of the box's 100, same dz.  Two
    runs of ONE schedule drift apart with every slice (the order of the LDS atomics): measured between runs of
    HPS_EARLY_INIT=0, worst component, 100 slices: 5.5e-13 .. 7.1e-13 at 128^2, but 0.8e-12 .. 1.1e-12 at 128 x 192, whose
    stretched cells take 291 V-cycles against 199 -- no room under 1e-12 there.  So only the cases that are about the whole
    step run it; the others run the short box, where the pass rides 39 times (odd, as after the whole step's 99)."""
    d = decks.blowout_wake()
    d.update(nx=nx, ny=ny, n_steps=1)
    if short:
        d.update(nz=40, lo=(-8.0, -8.0, -2.4), hi=(8.0, 8.0, 2.4))
    d.update(kw)
    return d


def _engine(api, deck, early, fusion=False):
    """one engine created with HPS_EARLY_INIT set (the library reads the switch when the engine is created)"""
    old = os.environ.get("HPS_EARLY_INIT")
    os.environ["HPS_EARLY_INIT"] = "1" if early else "0"
    try:
        e = api.SliceEngine(deck, tile_size=16, sort_period=7)
    finally:
        if old is None:
            del os.environ["HPS_EARLY_INIT"]
        else:
            os.environ["HPS_EARLY_INIT"] = old
    if fusion:
        e.set_fusion(True)
    return e


def _slices(e, deck, first, count):
    """`count` slices from the `first`-th one of the step on (0 = the head of the box)"""
    for k in range(deck["nz"] - 1 - first, deck["nz"] - 1 - first - count, -1):
        e.solve_slice(k)


def _state(e):
    return e.slab(), e.particles()


def _assert_same(a, b, names, what):
    (sa, (ra, va)), (sb, (rb, vb)) = a, b
    assert sa.shape == sb.shape, what
    for c, nm in enumerate(names):
        sc = max(np.abs(sb[c]).max(), 1e-300)
        err = np.abs(sa[c] - sb[c]).max()
        assert err <= TOL * sc, (what, nm, err / sc)
    assert ra.shape == rb.shape and np.array_equal(np.sort(va), np.sort(vb)), what
    assert np.abs(ra - rb).max() <= TOL * np.abs(rb).max(), what


_OFF = {}


def _off_run(api, key, deck, stops=(), steps=1, fusion=False):
    """The run with HPS_EARLY_INIT=0, computed once per deck: its state after each of `stops` slices of the first step and at
    the end of every step (reading the slab between slices is what the deferred shift has always allowed)."""
    if key not in _OFF:
        e = _engine(api, deck, False, fusion)
        out = {}
        for s in range(steps):
            e.begin_step()
            done = 0
            for n in (sorted(stops) if s == 0 else []):
                _slices(e, deck, done, n - done)
                done = n
                out[n] = _state(e)
            _slices(e, deck, done, deck["nz"] - done)
            out[("end", s)] = _state(e)
        assert e.stats()["early_init"] == 0
        out["names"] = e.comp_names()
        _OFF[key] = out
    return _OFF[key]


STOPS = (51, 52)      # an odd and an even number of ridden slices; the beam (|z| < 5.9 of 6) has particles on both


@pytest.mark.parametrize("nx,ny", [(128, 128), (128, 192)])
def test_on_against_off(api, nx, ny):
    """One whole step at 128^2, and 128 x 192 on the short box: the pass rides on every slice but the last, the results are
    those of the launches of its own."""
    info = api.MultiGrid(nx, ny, 16.0 / nx, 16.0 / ny).info()
    assert info["lowv"] == "v3" and info["lowv_begin"] >= 1, info      # a smoothed level above a k_lower_v3 lower V
    deck = _deck(nx, ny, short=(nx != ny))
    off = _off_run(api, (nx, ny), deck, STOPS if nx == ny else ())
    e = _engine(api, deck, True)
    e.begin_step()
    _slices(e, deck, 0, deck["nz"])
    assert e.stats()["early_init"] == deck["nz"] - 1
    _assert_same(_state(e), off[("end", 0)], off["names"], "end of the step")


@pytest.mark.parametrize("stop", STOPS)
def test_observed_at_either_parity(api, stop):
    """slab() and particles() after an odd / an even number of ridden slices show the slice just solved, and the run that goes
    on from there ends as the undisturbed one."""
    deck = _deck()
    off = _off_run(api, (128, 128), deck, STOPS)
    e = _engine(api, deck, True)
    e.begin_step()
    _slices(e, deck, 0, stop)
    assert e.stats()["early_init"] == stop
    _assert_same(_state(e), off[stop], off["names"], f"after {stop} slices")
    _slices(e, deck, stop, deck["nz"] - stop)
    assert e.stats()["early_init"] == deck["nz"] - 1
    _assert_same(_state(e), off[("end", 0)], off["names"], "end of the step")


def test_observed_after_every_slice(api):
    deck = _deck()
    off = _off_run(api, (128, 128), deck, STOPS)
    e = _engine(api, deck, True)
    e.begin_step()
    for n in range(deck["nz"]):
        _slices(e, deck, n, 1)
        e.sync()
        if n + 1 in STOPS:
            _assert_same(_state(e), off[n + 1], off["names"], f"after {n + 1} slices")
    assert e.stats()["early_init"] == deck["nz"] - 1
    _assert_same(_state(e), off[("end", 0)], off["names"], "end of the step")


def test_two_steps(api):
    """begin_step after an odd number (nz - 1 = 39) of ridden slices: the second step starts on the slab's own planes."""
    deck = _deck(short=True, n_steps=2)
    off = _off_run(api, "two steps", deck, steps=2)
    e = _engine(api, deck, True)
    for s in range(2):
        e.begin_step()
        _slices(e, deck, 0, deck["nz"])
        assert e.stats()["early_init"] == (s + 1) * (deck["nz"] - 1) and (deck["nz"] - 1) % 2 == 1
        if s == 1:
            _assert_same(_state(e), off[("end", s)], off["names"], f"end of step {s}")


@pytest.mark.parametrize("case", ["nodal", "generic_bottom", "lower_v_cc", "fusion", "deposit_rho"])
def test_paths_that_must_not_ride(api, case):
    """Grids whose lower V is not k_lower_v3 and the fused schedule keep the launches of their own (counter 0); a deck that
    deposits rho does ride, its rho plane included.  All of them give the results of HPS_EARLY_INIT=0."""
    nx, ny, kw, fusion, lowv = {"nodal": (127, 127, {}, False, "v-nodal"), "generic_bottom": (129, 129, {}, False, "bottom"),
                                "lower_v_cc": (132, 66, {}, False, "v-cc"), "fusion": (128, 128, {}, True, "v3"),
                                "deposit_rho": (128, 128, dict(deposit_rho=1), False, "v3")}[case]
    info = api.MultiGrid(nx, ny, 16.0 / nx, 16.0 / ny).info()
    assert info["lowv"] == lowv and info["cc"] == (nx % 2 == 0), info
    deck = _deck(nx, ny, short=True, **kw)
    off = _off_run(api, case, deck, fusion=fusion)
    e = _engine(api, deck, True, fusion)
    e.begin_step()
    _slices(e, deck, 0, deck["nz"])
    assert e.stats()["early_init"] == (deck["nz"] - 1 if case == "deposit_rho" else 0)
    if case == "deposit_rho":
        assert "rho" in off["names"] and np.abs(off[("end", 0)][0][off["names"].index("rho")]).max() > 0.0
    _assert_same(_state(e), off[("end", 0)], off["names"], case)
