"""The general fixed_ppc beam on the device (hps_engine_set_beam_fixed_ppc, hipace_amd/csrc/beam_init.hip).

* a constant program in the deck's flat-top window is the deck's own beam_profile = 1 beam bit for bit (Engine::init_beam is the
  yardstick), and the same run;
* arithmetic programs, random placement and the shapes that cross the kernel's seams: counts, order and positions bit-equal to the
  numpy restatement (tests/beam_init_reference.py), weights bit-equal to |hps_expr_eval_host * scale_fac|;
* momenta at the tolerance of tests/test_warm_plasma_gpu.py: |du_d| <= 1e-13 (u_std[d] + |u_mean[d]|) c;
* decks.beam_profile_expr of a Gaussian deck against the deck's beam: the weights differ by the rounding of three exp.

Beams are read back with beam_layout() and initial_beam_into(), as tests/test_host_beam_gpu.py does."""
import ctypes as C

import numpy as np
import pytest

from hipace_amd import decks, expr
from tests import beam_init_reference as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
HPS_ERR_ARG = 1


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def _beam(eng):
    """the engine's injected beam, head slice first: (7, n), offsets"""
    import torch
    n, off = eng.beam_layout()
    soa = np.empty((7, n))
    if n:
        blocks = torch.zeros(7 * n, dtype=torch.float64, device="cuda")
        eng.initial_beam_into(blocks)
        blk = blocks.cpu().numpy()
        for p in range(len(off) - 1):
            first, cnt = off[p], off[p + 1] - off[p]
            soa[:, first:first + cnt] = blk[7 * first:7 * (first + cnt)].reshape(7, cnt)
    return soa, off


def _deck(nx=21, ny=17, nz=9, ppc=(2, 2, 1), si=False, radius_cells=4.65, mean_cells=(1.15, -0.85), zcut=(1.35, 2.2), **kw):
    """the blowout deck on nx x ny x nz cells of its own cell size, a flat-top beam in a window given in cells: the radius around
    an off-axis mean, zmin / zmax between the sub-positions of a cell"""
    d = decks.blowout_wake_SI() if si else decks.blowout_wake()
    u = 10.0e-6 if si else 1.0
    h = 0.2 * u
    lo = (-0.5 * nx * h, -0.5 * ny * h, -0.5 * nz * h)
    d.update(nx=nx, ny=ny, nz=nz, lo=lo, hi=tuple(-v for v in lo), n_steps=1, beam_profile=1, beam_ppc=tuple(ppc),
             beam_density=2.0 * d["beam_density"], beam_radius=radius_cells * h, beam_pos_mean=(mean_cells[0] * h, mean_cells[1] * h, 0.0),
             beam_zmin=lo[2] + zcut[0] * h, beam_zmax=-lo[2] - zcut[1] * h)
    d.update(kw)
    return d


def _with(deck, text, constants=None, **kw):
    d = dict(deck, **decks.BEAM_INIT_DEFAULT)
    d.update(beam_density_expr=text, beam_density_constants=constants, **{"beam_" + k: v for k, v in kw.items()})
    return d


def _against_restatement(api, deck, text, constants=None, **kw):
    """engine of deck + program against the restatement: offsets, positions and weights bit for bit -> (soa, off, reference)"""
    eng = api.SliceEngine(_with(deck, text, constants, **kw), tile_size=0)
    soa, off = _beam(eng)
    prog = expr.compile_expr(text, ("x", "y", "z"), constants)
    ref = R.fixed_ppc_beam(deck, prog.evaluate, **kw)
    assert np.array_equal(off, ref["off"]), (off, ref["off"])
    for q in range(3):
        assert np.array_equal(soa[q], ref["soa"][q]), q
    _, _, _, scale = R.geometry(deck)
    host = api.Expression(prog).evaluate_host(soa[0], soa[1], soa[2]) if soa.shape[1] else np.empty(0)
    assert np.array_equal(soa[6], np.abs(host * scale))
    return soa, off, ref


# ---- flat top against the deck's own beam -------------------------------------------------------------------------------------

@pytest.mark.parametrize("ppc,si", [((1, 1, 1), False), ((2, 2, 1), True), ((2, 1, 3), False), ((2, 1, 3), True)])
def test_constant_program_is_the_decks_flattop_beam(api, ppc, si):
    deck = _deck(ppc=ppc, si=si)
    want, woff = _beam(api.SliceEngine(deck, tile_size=0))
    got, goff = _beam(api.SliceEngine(_with(deck, deck["beam_density"]), tile_size=0))
    full = deck["nx"] * deck["ny"] * int(np.prod(ppc))
    assert 0 < want.shape[1] and 0 < np.diff(woff).max() < full and (np.diff(woff) == 0).any()      # the radius cuts cells; empty slices
    assert np.array_equal(goff, woff)
    for q in range(7):
        assert np.array_equal(got[q], want[q]), q
    if ppc[2] == 3:      # zmin, zmax between the sub-positions: partly filled slices at both ends
        per = np.diff(woff)
        per = per[per > 0]
        assert per[0] < per.max() and per[-1] < per.max()


def test_constant_program_is_the_same_run(api):
    deck = _deck(nx=32, ny=32, nz=10, beam_density=1.0)
    a = api.SliceEngine(deck, tile_size=16)
    b = api.SliceEngine(_with(deck, "n0", dict(n0=deck["beam_density"])), tile_size=16)
    assert a.beam_layout()[0] == b.beam_layout()[0] > 100
    for e in (a, b):
        e.set_diagnostics(True)
        e.run_step()
    ca, cb = a.checksums(), b.checksums()
    for k in ca:      # the bar of test_deck_beam_through_the_host_entry_is_the_same_run
        assert abs(ca[k] - cb[k]) <= 1e-12 * abs(ca[k]), (k, ca[k], cb[k])
    assert ca["jz_beam"] != 0.0
    assert rel_err(b.slab(), a.slab()) < 1e-11


# ---- arithmetic programs ---------------------------------------------------------------------------------------------------

RING = "if(sqrt(x^2+y^2) > r0 and sqrt(x^2+y^2) < r1, n0*(1 + a*z), 0)"
RING_CONSTANTS = dict(r0=0.35, r1=0.8, n0=1.5, a=0.4)
COUPLED = "1 + 0.3*x*y + 0.05*z*x + if(x > 0.4 and y < -0.3, -5, 0)"      # couples x, y, z; removes a corner


@pytest.mark.parametrize("text,constants", [(RING, RING_CONSTANTS), (COUPLED, None)])
def test_arithmetic_program_against_the_restatement(api, text, constants):
    deck = _deck(nx=33, ny=17, nz=8, ppc=(2, 1, 3), mean_cells=(0.0, 0.0), radius_cells=5.3)
    soa, off, ref = _against_restatement(api, deck, text, constants)
    assert soa.shape[1] > 500 and (np.diff(off) == 0).any() and np.ptp(soa[6]) > 0.0
    for q in (3, 4, 5):      # a cold beam
        assert np.array_equal(soa[q], np.full(soa.shape[1], deck["beam_umean"][q - 3]))
    if text is RING:
        r = np.hypot(soa[0], soa[1])
        assert r.min() > 0.35 and r.max() < 0.8


def test_min_density_empty_beam_and_negative_density(api):
    deck = _deck(nx=16, ny=16, nz=8, mean_cells=(0.0, 0.0), radius_cells=6.1)
    step = "if(x > 0.3, 0.25, 1.0)"
    a, _, _ = _against_restatement(api, deck, step, min_density=0.25)       # a density equal to min_density is left out
    b, _, _ = _against_restatement(api, deck, step, min_density=0.2499)
    assert a.shape[1] > 0 and a[0].max() <= 0.3 and b[0].max() > 0.3 and b.shape[1] > a.shape[1]
    # a negative density with min_density = -inf: every point of the window, w = |density scale_fac|
    c, _, ref = _against_restatement(api, deck, "-2 - x*x", min_density=-np.inf)
    assert c.shape[1] == R.fixed_ppc_beam(deck, lambda x, y, z: 1.0 + 0.0 * x)["soa"].shape[1] and (ref["density"] < 0.0).all() and (c[6] > 0.0).all()
    # ... and with min_density = 0 it is a beam of no particle at all, which runs like a deck without a beam
    eng = api.SliceEngine(_with(deck, "-2 - x*x"), tile_size=16)
    n, off = eng.beam_layout()
    assert n == 0 and not off.any()
    eng.set_diagnostics(True)
    eng.run_step()
    ce = eng.checksums()      # (without a driver the plasma's fields are rounding residue: only the beam's planes are exact)
    assert all(ce[k] == 0.0 for k in ("jx_beam", "jy_beam", "jz_beam")) and np.isfinite(eng.slab()).all()


# ---- shapes that cross the kernel's seams -----------------------------------------------------------------------------------

SEAMS = {
    # (ny = 4: hps_engine_create takes no grid of fewer than 4 cells per side)
    "row_longer_than_a_workgroup": dict(nx=300, ny=4, nz=2, ppc=(2, 2, 1), radius_cells=140.3, mean_cells=(3.0, 0.0), zcut=(0.0, 0.0)),
    "odd_17_by_9": dict(nx=17, ny=9, nz=8, ppc=(2, 1, 3), radius_cells=3.9),
    "window_of_one_cell": dict(nx=17, ny=9, nz=8, ppc=(2, 2, 1), radius_cells=0.6, mean_cells=(2.0, -1.0), zcut=(3.1, 4.1)),
}


@pytest.mark.parametrize("case", sorted(SEAMS))
def test_seams_against_the_restatement(api, case):
    deck = _deck(**SEAMS[case])
    soa, off, _ = _against_restatement(api, deck, COUPLED if case != "window_of_one_cell" else "2 + x")
    if case == "row_longer_than_a_workgroup":
        assert np.diff(off).max() > 4 * 256                                      # several chunks per row, every row
    if case == "window_of_one_cell":
        assert soa.shape[1] == 4 and np.count_nonzero(np.diff(off)) == 1
        h = 0.2
        assert (np.floor((soa[0] - deck["lo"][0]) / h) == 17 // 2 + 2).all() and (np.floor((soa[1] - deck["lo"][1]) / h) == 9 // 2 - 1).all()


# ---- random placement --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("random_ppc", [(1, 1, 0), (0, 0, 1)])
def test_random_placement_against_the_restatement(api, random_ppc):
    deck = _deck(nx=21, ny=17, nz=9, ppc=(2, 2, 1), mean_cells=(0.0, 0.0), radius_cells=5.3)
    soa, off, ref = _against_restatement(api, deck, "1 + 0.2*x", random_ppc=random_ppc, seed=11)
    h, _, nppc, _ = R.geometry(deck)
    slot = ref["slot"]
    cell = [(slot // nppc) % deck["nx"], (slot // (nppc * deck["nx"])) % deck["ny"], slot // (nppc * deck["nx"] * deck["ny"])]
    for q in range(3):      # every particle inside its cell
        c = deck["lo"][q] + cell[q] * h[q]
        assert ((soa[q] >= c) & (soa[q] < c + h[q])).all(), q
        quarters = (soa[q] - c) / h[q] * 4.0                                       # the even lattice of ppc 2 2 1 sits on quarters of a cell
        assert (np.abs(quarters - np.round(quarters)) < 1e-9).all() != bool(random_ppc[q])
    # the selection is the cell corner's: whole cells, some of their particles beyond the radius
    xc, yc = deck["lo"][0] + cell[0] * h[0], deck["lo"][1] + cell[1] * h[1]
    assert (xc * xc + yc * yc <= deck["beam_radius"] ** 2).all() and (np.unique(slot // nppc, return_counts=True)[1] == nppc).all()
    assert (soa[0] ** 2 + soa[1] ** 2 > deck["beam_radius"] ** 2).any()
    # one seed, one beam; another seed, other positions
    again, _ = _beam(api.SliceEngine(_with(deck, "1 + 0.2*x", random_ppc=random_ppc, seed=11), tile_size=0))
    other, ooff = _beam(api.SliceEngine(_with(deck, "1 + 0.2*x", random_ppc=random_ppc, seed=12), tile_size=0))
    assert np.array_equal(again, soa)
    assert np.array_equal(ooff, off) and not np.array_equal(other[:3], soa[:3])


# ---- momenta -----------------------------------------------------------------------------------------------------------------

def test_momenta_against_the_restatement(api):
    deck = _deck(nx=21, ny=17, nz=9, ppc=(2, 1, 3), beam_umean=(0.1, -0.2, 2000.0))
    u_std = (0.3, 0.0, 2.0)
    soa, off, ref = _against_restatement(api, deck, COUPLED, u_std=u_std, seed=5)
    assert soa.shape[1] > 500
    assert np.array_equal(soa[4], np.full(soa.shape[1], -0.2))                    # u_std = 0: exactly u_mean c
    for d in (0, 2):      # the tolerance of tests/test_warm_plasma_gpu.py for its momenta
        tol = 1e-13 * (u_std[d] + abs(deck["beam_umean"][d]))
        err = np.abs(soa[3 + d] - ref["soa"][3 + d]).max()
        print(f"  u[{d}]: max |du| {err:.2e}, bound {tol:.2e}")
        assert err <= tol and np.std(soa[3 + d]) > 0.5 * u_std[d]


def test_momenta_in_si_units_carry_c(api):
    deck = _deck(nx=17, ny=9, nz=8, si=True, beam_umean=(0.0, 0.0, 100.0))
    u_std = (0.0, 0.5, 3.0)
    soa, _, ref = _against_restatement(api, deck, deck["beam_density"], u_std=u_std, seed=2)
    c = decks.SI["c"]
    assert soa.shape[1] > 100 and np.array_equal(soa[3], np.zeros(soa.shape[1]))
    for d in (1, 2):
        assert np.abs(soa[3 + d] - ref["soa"][3 + d]).max() <= 1e-13 * (u_std[d] + abs(deck["beam_umean"][d])) * c


def test_deviates_are_standard_normal(api):
    deck = _deck(nx=21, ny=17, nz=9, ppc=(4, 4, 3), radius_cells=100.0, zcut=(0.0, 0.0), beam_umean=(0.0, 0.0, 50.0))
    u_std = (0.5, 1.5, 4.0)
    soa, off = _beam(api.SliceEngine(_with(deck, 1.0, u_std=u_std, seed=3), tile_size=0))
    n = soa.shape[1]
    assert n == 21 * 17 * 9 * 48 >= 100000
    for d in range(3):
        dev = (soa[3 + d] - deck["beam_umean"][d]) / u_std[d]
        assert abs(dev.mean()) <= 5.0 / np.sqrt(n) and abs(dev.std() - 1.0) <= 5.0 / np.sqrt(n), (d, dev.mean(), dev.std())
    assert abs(np.corrcoef(soa[3], soa[4])[0, 1]) <= 5.0 / np.sqrt(n) and abs(np.corrcoef(soa[3], soa[5])[0, 1]) <= 5.0 / np.sqrt(n)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_usable(api):
    from hipace_amd import _lib
    L = _lib.lib()
    deck = _deck(nx=16, ny=16, nz=8, beam_density=1.0)
    eng = api.SliceEngine(deck, tile_size=16)
    n0 = eng.beam_layout()[0]
    good, keep = expr.compile_expr("1 + x*x", ("x", "y", "z")).c_struct()
    reads_t, keep_t = expr.compile_expr("1 + x*t").c_struct()
    vec = lambda *v: (C.c_double * 3)(*v)      # noqa: E731

    def refused(what, h, prog, min_density=0.0, u_std=None):
        st = L.hps_engine_set_beam_fixed_ppc(h, prog, min_density, u_std, None, 1)
        msg = L.hps_last_error().decode()
        assert st == HPS_ERR_ARG and what in msg, (what, st, msg)

    refused("null engine", None, C.byref(good))
    refused("null program", eng._h, None)
    refused("u_std", eng._h, C.byref(good), u_std=vec(0.0, -0.1, 0.0))
    refused("u_std", eng._h, C.byref(good), u_std=vec(0.0, 0.0, np.inf))
    refused("u_std", eng._h, C.byref(good), u_std=vec(np.nan, 0.0, 0.0))
    refused("min_density", eng._h, C.byref(good), min_density=np.nan)
    refused("min_density", eng._h, C.byref(good), min_density=np.inf)
    refused("variable", eng._h, C.byref(reads_t))
    assert eng.beam_layout()[0] == n0                                              # nothing changed
    zero_ppc = api.SliceEngine(dict(deck, beam_profile=-1, beam_ppc=(2, 0, 1)), tile_size=16)
    refused("beam_ppc", zero_ppc._h, C.byref(good))
    with pytest.raises(ValueError, match="cannot read t"):
        eng.set_beam_fixed_ppc("x*t")
    # still usable: the call goes through, whichever of the two entry points is called last holds, and the step runs
    eng.set_beam_fixed_ppc("1 + x*x")
    n1 = eng.beam_layout()[0]
    assert n1 == n0 > 0
    soa, _ = _beam(eng)
    eng.set_beam_particles(soa[:, :10])
    assert eng.beam_layout()[0] == 10
    eng.set_beam_fixed_ppc("1 + x*x", u_std=(0.1, 0.1, 0.1))
    assert eng.beam_layout()[0] == n1
    eng.set_diagnostics(True)
    eng.run_step()
    assert eng.checksums()["jz_beam"] != 0.0
    refused("before the first hps_engine_begin_step", eng._h, C.byref(good))


# ---- against numbers to be measured ---------------------------------------------------------------------------------------

# largest relative difference of the Gaussian weights between the program (the device's exp) and Engine::init_beam (the host's),
# measured on MI355X; the bound is four times that, for other libm builds, and never more than 64 eps
GAUSSIAN_MEASURED = 5.933e-16      # 2.67 eps
GAUSSIAN_BOUND = min(4.0 * GAUSSIAN_MEASURED, 64.0 * EPS)


def _gaussian_deck():
    d = _deck(nx=32, ny=32, nz=10, ppc=(2, 2, 1), mean_cells=(0.0, 0.0), radius_cells=13.1, zcut=(0.3, 0.3),
              beam_profile=0, beam_density=2.0, beam_pos_std=(0.5, 0.6, 0.45))      # the box spans +- 6.4, 5.3 and 2.2 sigma: no weight underflows
    return d


def test_gaussian_profile_as_a_program(api):
    deck = _gaussian_deck()
    text, constants = decks.beam_profile_expr(deck)
    a = api.SliceEngine(deck, tile_size=16)
    b = api.SliceEngine(_with(deck, text, constants), tile_size=16)
    want, woff = _beam(a)
    got, goff = _beam(b)
    assert want.shape[1] > 10000 and np.array_equal(goff, woff) and want[6].min() > 1e-30
    for q in range(6):
        assert np.array_equal(got[q], want[q]), q
    worst = (np.abs(got[6] - want[6]) / want[6]).max()
    print(f"  Gaussian weights, program against init_beam: max relative difference {worst:.3e} = {worst / EPS:.2f} eps, bound {GAUSSIAN_BOUND / EPS:.2f} eps")
    assert worst <= GAUSSIAN_BOUND
    # the one-step run holds the deck's field sums to the project's checksum bar
    for e in (a, b):
        e.set_diagnostics(True)
        e.run_step()
    ca, cb = a.checksums(), b.checksums()
    for k in ca:
        assert abs(ca[k] - cb[k]) <= 1e-9 * max(abs(ca[k]), 1e-300), (k, ca[k], cb[k])
    assert ca["jz_beam"] != 0.0


def test_moving_warm_beam_keeps_its_particles(api):
    deck = decks.beam_evolution()
    deck.update(nx=16, ny=16, nz=8, beam_ppc=(2, 2, 1), n_steps=2)
    text, constants = decks.beam_profile_expr(deck)
    eng = api.SliceEngine(_with(deck, text, constants, u_std=(1.0, 2.0, 10.0), seed=4), tile_size=0)
    soa0, off0 = _beam(eng)
    bnd, state = eng.beam_state()
    assert soa0.shape[1] > 100 and np.array_equal(bnd, off0) and np.array_equal(state, soa0)      # the global SoA is the blocks
    assert np.std(soa0[3]) > 0.5 and np.std(soa0[5]) > 5.0
    eng.set_insitu_beam()
    for _ in range(2):
        eng.run_step()
    bnd, state = eng.beam_state()
    assert bnd[-1] - bnd[0] == soa0.shape[1] and np.isfinite(state).all()
    assert not np.array_equal(state[0], soa0[0])                                   # it moved
    ins = eng.insitu_beam()
    assert ins["Np"].sum() == soa0.shape[1]
    assert abs(ins["sum(w)"].sum() - soa0[6].sum()) <= 1e-9 * soa0[6].sum()


def test_hollow_beam_deck_drives_a_wake_with_an_empty_axis(api):
    deck = decks.blowout_wake_hollow_beam()
    deck.update(nz=12, n_steps=1, lo=(-8.0, -8.0, -0.72), hi=(8.0, 8.0, 0.72), beam_zmin=-0.7, beam_zmax=0.7)
    eng = api.SliceEngine(deck, tile_size=16)
    soa, off = _beam(eng)
    r = np.hypot(soa[0], soa[1])
    assert soa.shape[1] > 200 and r.min() >= 0.6 and r.max() < 1.0
    eng.set_field_diagnostic(["Ez", "jz_beam"])
    eng.run_step()
    fd = eng.field_diagnostic()
    mid = slice(deck["nx"] // 2 - 1, deck["nx"] // 2 + 1)
    assert np.abs(fd["Ez"][:, mid, mid]).max() > 0.0
    assert np.abs(fd["jz_beam"][:, mid, mid]).max() == 0.0 and np.abs(fd["jz_beam"]).max() > 0.0
