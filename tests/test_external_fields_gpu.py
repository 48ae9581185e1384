"""beams.external_E / external_B as expression programs on the GPU: the device evaluator (api.Expression,
k_expr_eval) against the same routine on the host, the beam push with programs (k_beam_push<ORDER, true>) against the numpy
restatement of tests/external_field_reference.py and against the oracle, the step's physical time, and what must not move.

Shapes: 32 x 32 cells, 12 slices, a host beam of 333 particles (two 256-lane workgroups, the second partly filled, not a
multiple of the 64-lane wave), two slices empty at the start, 4 sub-cycles, 3 steps."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from hipace_amd import decks
from tests import external_field_reference as R
from tests.test_external_fields_cpu import CONSTS, TABLE

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Device against host (the C library's libm) per transcendental function, over POINTS below: the deviation measured on an
# MI355X in ulps of the result, and the bound asserted = 4 x that, rounded up to whole ulps (the margin is for arguments the
# points do not hit).
#            text                       measured  bound
FUNCTIONS = [
    ("pow(abs(x) + 0.1, y)",            1, 4),
    ("exp(x)",                          1, 4),
    ("log(abs(x) + 0.01)",              1, 4),
    ("log10(abs(x) + 0.01)",            2, 8),
    ("sin(3*x)",                        1, 4),
    ("cos(3*x)",                        1, 4),
    ("tan(x/2)",                        1, 4),
    ("asin(x/2)",                       1, 4),
    ("acos(x/2)",                       1, 4),
    ("atan(x)",                         1, 4),
    ("atan2(y, x)",                     1, 4),
    ("sinh(x)",                         2, 8),
    ("cosh(x)",                         1, 4),
    ("tanh(x)",                         2, 8),
    ("erf(x)",                          1, 4),
]
# the unchanged deck-slope path (ext_E_slope, ext_Ez_slope; k_beam_push<ORDER, false>) against the restatement on the beam of
# the trajectory test: the largest deviation of any quantity over that quantity's maximum, measured on an MI355X
D0_MEASURED = 4.1e-16      # (1.9e-16 .. 4.1e-16 over the sixteen cases; the program path: 2.9e-16 .. 3.5e-16)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


@pytest.fixture(scope="module")
def points():
    rng = np.random.default_rng(11)
    x, y, z, t = [rng.uniform(-2.0, 2.0, 1000) for _ in range(4)]
    x[:4] = [0.0, -0.0, 1.0, -1.0]
    y[:4] = [0.0, 1.0, 1.0, -1.0]
    return x, y, z, t


def _device(api, ex, pts):
    import torch
    ten = [torch.tensor(p, dtype=torch.float64, device="cuda") for p in pts]
    out = ex(*ten)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ulps(a, b):
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~ok & ~np.isnan(a)], b[~ok & ~np.isnan(b)])
    s = np.maximum(np.maximum(np.abs(a[ok]), np.abs(b[ok])), np.finfo(float).tiny)
    return float((np.abs(a[ok] - b[ok]) / np.spacing(s)).max()) if ok.any() else 0.0


# ---- 1. the evaluator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [k for k, r in enumerate(TABLE) if r[2]])
def test_arithmetic_and_select_programs_are_bit_equal_to_the_host(api, points, row):
    """every row of the CPU table made of + - * / sqrt, comparisons, selects and their kin (the depth-16 and the
    255-instruction program among them): k_expr_eval and hps_expr_eval_host run one routine that rounds every operation once"""
    ex = api.Expression(TABLE[row][0], constants=CONSTS)
    with np.errstate(all="ignore"):
        host = ex.evaluate_host(*points)
    dev = _device(api, ex, points)
    assert np.array_equal(dev, host, equal_nan=True), TABLE[row][0]


@pytest.mark.parametrize("row", range(len(FUNCTIONS)))
def test_transcendental_functions_stay_within_their_measured_ulps(api, points, row):
    text, measured, bound = FUNCTIONS[row]
    ex = api.Expression(text)
    with np.errstate(all="ignore"):
        host = ex.evaluate_host(*points)
    u = _ulps(_device(api, ex, points), host)
    print(f"ULPS {text!r}: device against host {u:.3f} ulp (recorded {measured}, bound {bound})")
    assert bound is not None, "no bound recorded for this function"
    assert bound == math.ceil(4 * measured) and bound <= 16
    assert u <= bound, (text, u, bound)


def test_zero_elements_and_a_depth_one_program(api, points):
    import torch
    ex = api.Expression("x")                      # depth 1: no LDS at all
    assert ex.depth == 1
    assert np.array_equal(_device(api, ex, points), points[0])
    empty = [torch.empty(0, dtype=torch.float64, device="cuda") for _ in range(4)]
    assert api.Expression("sin(x) + y")(*empty).numel() == 0
    one = api.Expression("2.5")                    # a constant: no variable is read
    assert np.array_equal(_device(api, one, points), np.full(1000, 2.5))
    two = api.Expression("a*b + a", variables=("a", "b"))
    assert np.array_equal(_device(api, two, points[:2]), two.evaluate_host(*points[:2]))


# ---- 2. trajectories in vacuum ------------------------------------------------------------------------------------------
def _run_engine(api, deck, soa, fields=None):
    d = dict(deck)
    if fields is not None:
        d["beam_external_fields"] = fields
    eng = api.SliceEngine(d, tile_size=0)
    assert eng.set_beam_particles(soa) == 0
    eng.set_diagnostics(True)
    for _ in range(deck["n_steps"]):
        eng.run_step()
    bnd, state = eng.beam_state()
    spin = eng.beam_spin() if deck.get("beam_spin_tracking", 0) else None
    return eng, bnd, state, spin


def _deviation(bnd, state, spin, ref):
    """-> per quantity (x y z ux uy uz w, then sx sy sz with spin): largest deviation over the quantity's maximum"""
    got, gs = R.match_engine_state(bnd, state, ref, spin)
    want = ref.state()
    assert not np.isnan(got).any()
    dev = []
    for q in range(7):
        scale = np.abs(want[q]).max()
        dev.append(np.abs(got[q] - want[q]).max() / scale if scale > 0 else float(np.abs(got[q]).max()))
    if spin is not None:
        for q in range(3):
            dev.append(np.abs(gs[q] - ref.s[q]).max() / np.abs(ref.s[q]).max())
    return np.array(dev)


@pytest.mark.parametrize("rr", [False, True])
@pytest.mark.parametrize("spin", [False, True])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_trajectories_in_vacuum_follow_the_restatement(api, order, spin, rr):
    """Zero-weight host beam, no plasma: every grid field is exactly zero and the programs are the only force.  Every particle
    -- the one absorbed at the wall, the ones that slip into the next slice in mid-step and finish their sub-cycles there, the
    rest -- against the restatement.  Bound: 8 d0 + 1e-14 of each quantity's maximum, d0 = the deviation of the unchanged
    deck-slope path on the same beam in a linear field of like size, measured in this test (8: six components instead of
    three, and the extra rounding per component)."""
    deck = R.vacuum_deck(order, spin, rr)
    soa = R.vacuum_beam()
    # the deck-slope path, E = (0.3 x, 0.2 y, 0.1 z)
    sdeck = dict(deck, ext_E_slope=R.LINEAR_SLOPES[:2], ext_Ez_slope=R.LINEAR_SLOPES[2])
    sref = R.BeamRestatement(sdeck, soa)
    for _ in range(deck["n_steps"]):
        sref.run_step()
    _, bnd, state, sp = _run_engine(api, sdeck, soa)
    d0 = float(_deviation(bnd, state, sp, sref).max())
    # the programs
    ref = R.BeamRestatement(deck, soa, R.compile_fields(R.FIELDS_E, R.FIELDS_B))
    for _ in range(deck["n_steps"]):
        ref.run_step()
    assert ref.n_absorbed == 1 and ref.n_slipped_mid_step >= 3 and not (ref.islice < 0).any()
    assert (ref.islice == 11).sum() == 0 and ref.alive.sum() == soa.shape[1] - 1
    eng, bnd, state, sp = _run_engine(api, deck, soa, dict(E=R.FIELDS_E, B=R.FIELDS_B))
    dev = _deviation(bnd, state, sp, ref)
    print(f"D0 order {order} spin {spin} rr {rr}: slope path {d0:.3e}, program path {dev.max():.3e} (recorded d0 {D0_MEASURED})")
    assert d0 < 1e-12                              # the slope path itself follows the restatement
    assert np.all(dev <= 8 * d0 + 1e-14), (dev, d0)
    cs = eng.checksums()
    assert all(v == 0.0 for v in cs.values()), cs  # zero weights, no plasma: nothing on the grid


# ---- 3. against the oracle with a wake ----------------------------------------------------------------------------------
def test_programs_with_a_wake_match_the_oracle_run_with_the_slopes(api, oracle):
    """the deck of test_beam_slipping_matches_oracle with a plasma: the oracle with ext_E_slope = (0.3, 0.2), the engine with
    the slopes zeroed and E = ("0.3*x", "0.2*y", "0"); checksums and every particle to 1e-9"""
    deck = decks.beam_evolution()
    deck.update(nz=12, lo=(-2.0, -2.0, -2.4), hi=(2.0, 2.0, 2.4), beam_zmin=-1.0, beam_zmax=1.6, beam_umean=(0.0, 0.0, 1.2),
                beam_density=1.0e-3, n_steps=6, dt=0.9, beam_n_subcycles=4, ext_E_slope=(0.3, 0.2), plasma_ppc=(1, 1), plasma_density=1.0)
    ref = oracle.Engine(deck)
    ref.run()
    pdeck = dict(deck, ext_E_slope=(0.0, 0.0), beam_external_fields=dict(E=("0.3*x", "0.2*y", "0")))
    eng = api.SliceEngine(pdeck, tile_size=0)
    eng.set_diagnostics(True)
    for _ in range(deck["n_steps"]):
        eng.run_step()
    bnd, soa = eng.beam_state()
    nz = deck["nz"]
    moved, n0 = 0, oracle.Engine(deck)
    for p in range(nz):
        want = ref.beam_slice(nz - 1 - p)
        got = soa[:, bnd[p]:bnd[p + 1]]
        assert got.shape == want.shape, (p, got.shape, want.shape)
        moved += abs(want.shape[1] - n0.beam_slice(nz - 1 - p).shape[1])
        if want.shape[1]:
            ko = np.lexsort((want[1], want[0])); kg = np.lexsort((got[1], got[0]))
            assert np.abs(got[:, kg] - want[:, ko]).max() <= 1e-9 * np.abs(want).max()
    assert moved > 0
    cs, rs = eng.checksums(), ref.checksums()
    assert rs["Ez"] > 0 and rs["ExmBy"] > 0        # there is a wake
    for k, v in rs.items():
        assert abs(cs[k] - v) <= 1e-9 * max(abs(v), 1e-300), (k, cs[k], v)


def test_beam_evolution_parsed_matches_reference_checksums(api):
    """tests/beam_evolution.1Rank.sh with beams.external_E = .5*x .5*y 0. as the script writes it, against the reference's JSON"""
    deck = decks.beam_evolution_parsed()
    gold = json.load(open(os.path.join(GOLD, "beam_evolution.1Rank.json")))["lev=0"]
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_diagnostics(True)
    for _ in range(deck["n_steps"]):
        eng.run_step()
    cs = eng.checksums()
    for k, v in gold.items():
        if v == 0.0:
            assert cs[k] == 0.0, (k, cs[k])
        else:
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (k, cs[k], v)


# ---- 4. time ------------------------------------------------------------------------------------------------------------
E0_T, W_T, UZ0 = 0.5, 1.3, 100.0


def _rest_beam(n=333):
    rng = np.random.default_rng(5)
    soa = np.zeros((7, n))
    soa[0], soa[1] = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    soa[2] = rng.uniform(-2.3, 2.3, n)
    soa[5] = UZ0
    return soa


def _time_deck(**kw):
    d = R.vacuum_deck(order=2)
    d.update(n_steps=4, beam_n_subcycles=8, beam_external_fields=dict(E=(0, 0, "E0*cos(w*t)"), constants=dict(E0=E0_T, w=W_T)))
    d.update(kw)
    return d


def _uz_after(times, dts):
    """uz0 + (q/m) sum dt_k E0 cos(w t_k): the particles are at rest transversely and B = 0, so every sub-cycle of a step adds
    (dt/8) q/m Ez(t of the step)"""
    uz, out = UZ0, []
    for t, dt in zip(times, dts):
        uz = uz + (-1.0) * dt * (E0_T * np.cos(W_T * t))
        out.append(uz)
    return out


def _check_uz(eng, want):
    """32 additions of one rounding each (2^-53 of uz ~ 100 each: 4e-15 relative in all) and a cosine good to a few ulps: 1e-13"""
    _, soa = eng.beam_state()
    assert soa.shape[1] == 333
    assert np.abs(soa[5] - want).max() <= 1e-13 * abs(want), (np.abs(soa[5] - want).max(), want)
    assert np.all(soa[3] == 0.0) and np.all(soa[4] == 0.0)


def test_the_field_sees_the_time_of_the_step_fixed_dt(api):
    deck = _time_deck()
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_beam_particles(_rest_beam())
    want = _uz_after([deck["dt"] * k for k in range(4)], [deck["dt"]] * 4)
    assert abs(want[3] - want[0]) > 0.1
    for s in range(4):
        eng.run_step()
        _check_uz(eng, want[s])


def test_the_field_sees_the_time_it_was_given_adaptive(api):
    """hipace.dt = adaptive: time and dt of every step come through set_time -- not step*dt"""
    deck = _time_deck(dt=0.0, dt_adaptive=1)
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_beam_particles(_rest_beam())
    times, dts = [0.0, 0.7, 1.9, 2.2], [0.7, 1.2, 0.3, 0.5]
    want = _uz_after(times, dts)
    for s in range(4):
        eng.set_time(times[s], dts[s])
        eng.run_step()
        _check_uz(eng, want[s])


def test_every_engine_in_flight_sees_its_own_steps_time(api):
    """two time steps in flight (run_lanes): stage 0 runs steps 0 and 2, stage 1 steps 1 and 3, each at dt*step"""
    import torch
    from hipace_amd.pipeline import run_lanes
    deck = _time_deck()
    soa = _rest_beam()

    def engine():
        e = api.SliceEngine(deck, tile_size=0)
        e.set_beam_particles(soa)
        return e
    want = _uz_after([deck["dt"] * k for k in range(4)], [deck["dt"]] * 4)
    seen = []

    def on_end(step, e):
        _check_uz(e, want[step])
        seen.append(step)
    run_lanes([engine(), engine()], 0, 1, 4, torch.device("cuda", 0), on_step_end=on_end)
    assert sorted(seen) == [0, 1, 2, 3]


# ---- 5. nothing moves that should not -----------------------------------------------------------------------------------
# Bit-identity is asserted where the engine itself is reproducible bit by bit: the beam's particles (a per-particle push) in a
# deck whose grid fields are exactly zero.  With a plasma, or a beam that deposits, the depositions add with floating-point
# atomics and two runs of ONE deck differ in the last bits of every checksum (measured here on the static blowout deck: jx
# 143.82972270703834 against 143.82972270703831, Psi 7e-16 relative), and the partition leaves the order inside a slice open;
# there the comparison is per slice as sets, to the 1e-9 that smoke() and the parity tests hold two such runs to.
def _sorted_state(eng, nz):
    bnd, soa = eng.beam_state()
    out = []
    for p in range(nz):
        blk = soa[:, bnd[p]:bnd[p + 1]]
        out.append(blk[:, np.lexsort((blk[2], blk[1], blk[0]))])
    return bnd, out


def test_an_all_zero_entry_changes_nothing(api):
    zero = dict(E=(0, "0.", "kp - kp"), B=("0", 0.0, "0*pi"), constants=dict(kp=2.0))
    # in vacuum, zero weights, the deck's slopes: bit-identical, particle by particle
    vdeck = dict(R.vacuum_deck(), ext_E_slope=R.LINEAR_SLOPES[:2], ext_Ez_slope=R.LINEAR_SLOPES[2])
    out = []
    for entry in (None, zero):
        eng, _, _, _ = _run_engine(api, vdeck, R.vacuum_beam(), entry)
        assert entry is None or all(p.is_zero for three in eng.beam_external_fields for p in three)
        out.append((_sorted_state(eng, vdeck["nz"]), eng.checksums()))
    (b0, s0), c0 = out[0]
    (b1, s1), c1 = out[1]
    assert np.array_equal(b0, b1) and all(np.array_equal(u, v) for u, v in zip(s0, s1)) and c0 == c1
    # with a wake
    deck = decks.beam_evolution()
    deck.update(nz=12, lo=(-2.0, -2.0, -2.4), hi=(2.0, 2.0, 2.4), beam_zmin=-1.0, beam_zmax=1.6, beam_umean=(0.0, 0.0, 1.2),
                beam_density=1.0e-3, n_steps=3, dt=0.9, beam_n_subcycles=4, ext_E_slope=(0.3, 0.2), plasma_ppc=(1, 1), plasma_density=1.0)
    out = []
    for entry in (None, zero):
        d = dict(deck) if entry is None else dict(deck, beam_external_fields=entry)
        eng = api.SliceEngine(d, tile_size=0)
        eng.set_diagnostics(True)
        for _ in range(deck["n_steps"]):
            eng.run_step()
        out.append((_sorted_state(eng, deck["nz"]), eng.checksums()))
    (b0, s0), c0 = out[0]
    (b1, s1), c1 = out[1]
    assert np.array_equal(b0, b1) and c0["Ez"] > 0
    for u, v in zip(s0, s1):
        assert u.shape == v.shape and (u.size == 0 or np.abs(u - v).max() <= 1e-9 * np.abs(u).max())
    for k, v in c0.items():
        assert abs(c1[k] - v) <= 1e-9 * abs(v), (k, c1[k], v)


def test_a_static_beam_ignores_the_programs(api):
    """hipace.dt = 0: the beam is never pushed; programs are accepted and change nothing, a SALAME deck included.  The static
    beam bit by bit; the checksums of two runs of one deck differ by the order of the depositions' atomics only -- the bound
    smoke() holds the engine to, 1e-9; the weights SALAME leaves are ratios of such sums: ten times the 1.45e-13 that
    tests/test_salame_gpu.py measured between two runs of that deck."""
    for base, w_tol in ((dict(decks.blowout_wake(), nz=12, lo=(-8.0, -8.0, -0.72), hi=(8.0, 8.0, 0.72), n_steps=2), 0.0),
                        (decks.salame_grid_current(), 1.45e-12)):
        out = []
        for entry in (None, dict(E=R.FIELDS_E, B=R.FIELDS_B)):
            d = dict(base) if entry is None else dict(base, beam_external_fields=entry)
            eng = api.SliceEngine(d)
            eng.set_diagnostics(True)
            for _ in range(base["n_steps"]):
                eng.run_step()
            out.append((eng.beam_state(), eng.checksums()))
        (b0, s0), c0 = out[0]
        (b1, s1), c1 = out[1]
        assert np.array_equal(b0, b1) and np.array_equal(s0[:6], s1[:6])
        assert np.abs(s0[6] - s1[6]).max() <= w_tol * np.abs(s0[6]).max()
        for k, v in c0.items():
            assert abs(c1[k] - v) <= 1e-9 * abs(v), (k, c1[k], v)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(api):
    from hipace_amd import _lib, expr
    L = _lib.lib()
    deck = R.vacuum_deck()
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_beam_particles(R.vacuum_beam())
    eng.set_beam_external_fields(E=("x", "y", "z"))                  # twice before the first step: the second call replaces
    eng.set_beam_external_fields(E=R.FIELDS_E, B=R.FIELDS_B)
    # a program that fails the check: E[1] ends with two values
    good, keep = expr.compile_expr("x").c_struct()
    ins = (_lib.ExprIns * 2)(_lib.ExprIns(expr.OP["var"], 0), _lib.ExprIns(expr.OP["var"], 1))
    bad = _lib.Expr(2, 0, C.cast(ins, C.POINTER(_lib.ExprIns)), None)
    three = (_lib.Expr * 3)(good, bad, good)
    assert L.hps_engine_set_beam_external_fields(eng._h, three, None) == 1
    err = L.hps_last_error().decode()
    assert err.startswith("hps_engine_set_beam_external_fields: E[1]: ") and "exactly one value" in err
    three = (_lib.Expr * 3)(good, good, good)
    assert L.hps_engine_set_beam_external_fields(None, three, None) == 1 and "null engine" in L.hps_last_error().decode()
    eng.begin_step()
    with pytest.raises(_lib.HpsError, match="hps_engine_set_beam_external_fields: call before the first hps_engine_begin_step"):
        eng.set_beam_external_fields(E=("x", "y", "z"))
    for islice in range(deck["nz"] - 1, -1, -1):
        eng.solve_slice(islice)
    # the refused calls changed nothing: the step ran with FIELDS_E / FIELDS_B
    ref = R.BeamRestatement(deck, R.vacuum_beam(), R.compile_fields(R.FIELDS_E, R.FIELDS_B))
    ref.run_step()
    bnd, state = eng.beam_state()
    got, _ = R.match_engine_state(bnd, state, ref)
    assert np.abs(got[3] - ref.ux).max() <= 1e-12 * np.abs(ref.ux).max()
    with pytest.raises(ValueError, match="three components"):
        api.SliceEngine(dict(deck, beam_external_fields=dict(E=("x", "y"))), tile_size=0)
    with pytest.raises(ValueError, match="unknown entries"):
        api.SliceEngine(dict(deck, beam_external_fields=dict(E=("x", "y", "z"), D=("x", "y", "z"))), tile_size=0)
