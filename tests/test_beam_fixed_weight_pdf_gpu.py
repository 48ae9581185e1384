"""The fixed_weight_pdf beam on the device (hps_engine_set_beam_fixed_weight_pdf, hipace_amd/csrc/beam_init.hip) against
the numpy restatement tests/beam_fixed_weight_pdf_reference.py, which takes the pdf at the edges from the library's host routine.
Engine A takes the device beam, engine B the restatement's particles through set_beam_particles(allow_outside=True); B's
beam_state() is the restatement bit for bit, so A is held against both.

* offsets, the two left-out counts, the order and every draw's sub-slice s: exact (tests/test_beam_fixed_weight_pdf_cpu.py keeps
  every case 1e-9 clear of the cuts);
* x - X, y - Y and u: within 1e-13 (std + |mean|) at the draw's z -- times c for u --, the bound of
  tests/test_beam_fixed_weight_gpu.py for Box-Muller deviates; z within 1e-13 (zs + |z|), bit for bit with a constant pdf;
* weights: within weight_roundings(ns) eps, the counted roundings of the chain;
* every program bit for bit at the device's z, for arithmetic programs.

Maxima measured on the MI355X (in units of the bound; printed by every test): z 0 in every case, both branches; gaussian x 4.8e-3,
y 4.0e-3, u 1.9e-3; constant 5.2e-3; windowed 8.1e-3; two bunches 4.7e-3; ratio 1 and 3 6.1e-3; programs 5.6e-3; symmetrized
6.7e-3; focus 3.7e-3; radius with density 3.0e-3; total_charge (SI) 8.0e-3; weights equal bit for bit."""
import numpy as np
import pytest

from hipace_amd import decks
from tests import beam_fixed_weight_pdf_reference as R

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
CASES = R.cases()


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def _pe_of(api, deck, beam):
    """the pdf at the edges from the library's own host routine"""
    return api.Expression(beam["pdf"], ("z",), beam.get("constants")).evaluate_host(R.edges(deck, beam.get("pdf_ref_ratio", 4)))


def _reference(api, deck, beam):
    ref = R.fixed_weight_pdf_beam(deck, _pe_of(api, deck, beam), **beam)
    return ref, R.binned(deck, ref)


def _pair(api, deck, beam):
    """engines A and B of (deck, beam) -> (A's beam_state soa, the restatement as binned, the restatement in draw order, A)"""
    ref, want = _reference(api, deck, beam)
    a = api.SliceEngine(deck, tile_size=0)
    left = a.set_beam_fixed_weight_pdf(**beam)
    assert left == (want["n_invalid"], want["n_outside"]), (left, want["n_invalid"], want["n_outside"])
    b = api.SliceEngine(deck, tile_size=0)
    assert b.set_beam_particles(ref["soa"][:, ref["valid"]], allow_outside=True) == want["n_outside"]
    (na, offa), (nb, offb) = a.beam_layout(), b.beam_layout()
    assert na == nb == want["soa"].shape[1] and np.array_equal(offa, offb) and np.array_equal(offa, want["off"])
    assert na + sum(left) == beam["num_particles"]
    bnda, soa = a.beam_state()
    bndb, sob = b.beam_state()
    assert np.array_equal(bnda, offa) and np.array_equal(bndb, offa)
    assert np.array_equal(sob, want["soa"])
    tab = ref["table"]
    assert a.beam_uz_moments == (tab["uz_mean"], tab["uz_std"])
    return soa, want, ref, a


def _hold(name, deck, beam, soa, want, ref, z_exact=False):
    """rows in order against the restatement at the bounds of the module's docstring; prints the maxima in units of the bound"""
    c = decks.SI["c"] if deck.get("si_units", 0) else 1.0
    m = 4 if beam.get("do_symmetrize") else 1
    draw = (want["i"] - ref["i"][0]).astype(np.int64)
    tab = ref["table"]
    # the sub-slice of every kept draw, from the device's own z
    zs, lo_z = tab["zs"], deck["lo"][2]
    s_dev = np.floor((soa[2] - lo_z) / zs + 1e-6).astype(np.int64)      # (z is never below its sub-slice's lower edge)
    s_ref = ref["s"][draw]
    on_edge = np.abs((soa[2] - lo_z) / zs - np.rint((soa[2] - lo_z) / zs)) < 1e-6
    assert np.array_equal(s_dev[~on_edge], s_ref[~on_edge]) and on_edge.sum() <= 1e-3 * max(soa.shape[1], 1000), name
    bound = [1e-13 * (ref["sx"][draw] + np.abs(ref["X"][draw])), 1e-13 * (ref["sy"][draw] + np.abs(ref["Y"][draw])),
             1e-13 * (zs + np.abs(ref["z"][draw]))]
    bound += [1e-13 * (ref["us"][d][draw] + np.abs(ref["um"][d][draw])) * c for d in range(3)]
    worst = []
    for r in range(6):
        err = np.abs(soa[r] - want["soa"][r])
        if r == 2 and z_exact:
            assert np.array_equal(soa[2], want["soa"][2])
        worst.append(float((err / np.maximum(bound[r], 1e-300)).max()) if err.size else 0.0)
        assert (err <= bound[r]).all(), (name, r, worst[-1])
    werr = np.abs(soa[6] / ref["weight"] - 1.0).max() / EPS if soa.shape[1] else 0.0
    print(f"{name}: max error / bound of x y z ux uy uz = {' '.join(f'{v:.2e}' for v in worst)}; weight {werr:.2f} eps (m = {m})")
    assert werr <= R.weight_roundings(tab["ns"])
    return worst


def _case(api, name, **kw):
    deck, beam = CASES[name]
    soa, want, ref, eng = _pair(api, deck, beam)
    _hold(name, deck, beam, soa, want, ref, **kw)
    return deck, beam, soa, want, ref, eng


# ---- 1. the pdfs --------------------------------------------------------------------------------------------------------------

def test_gaussian_pdf_particle_by_particle(api):
    deck, beam, soa, want, ref, _ = _case(api, "gaussian")
    off = want["off"]
    assert soa.shape[1] == 4096 and np.diff(off).min() > 0
    assert 0.2 < ref["taylor"].mean() < 0.8      # both branches
    assert np.ptp(ref["X"]) > 0.1 and np.ptp(ref["sx"]) > 0.05 and np.ptp(ref["um"][2]) > 10.0 and ref["us"].min() > 0.0
    for p in range(deck["nz"]):      # slices head first, ascending draw inside a slice
        i = want["i"][off[p]:off[p + 1]]
        assert (np.diff(i) > 0).all()
        hi = deck["hi"][2] - 0.2 * p
        assert (soa[2, off[p]:off[p + 1]] <= hi).all() and (soa[2, off[p]:off[p + 1]] >= hi - 0.2 - 1e-12).all()


def test_constant_pdf_is_bit_equal_in_z(api):
    deck, beam, soa, want, ref, _ = _case(api, "constant", z_exact=True)
    assert ref["taylor"].all() and np.bincount(ref["s"], minlength=32).min() > 60


def test_windowed_pdf(api):
    deck, beam, soa, want, ref, _ = _case(api, "windowed")
    lw, zs = ref["table"]["lw"], ref["table"]["zs"]
    assert lw[0] == 0.0 and lw[-1] == 0.0 and (lw[ref["s"]] > 0.0).all()
    first, last = np.flatnonzero(lw > 0.0)[[0, -1]]      # the two sub-slices with a zero edge: the square-root branch from 0
    # (the table's profile is linear inside a sub-slice: the window's ends are as sharp as the sub-slices that hold them)
    assert (first, last) == (5, 28) and soa[2].min() > -0.8 + 5 * zs and soa[2].max() < -0.8 + 29 * zs
    assert (ref["s"] == first).any() and (ref["s"] == last).any() and not ref["taylor"][(ref["s"] == first) | (ref["s"] == last)].any()
    # the tail slice, z < -0.6, is empty; the head slice, z >= 0.6, holds the draws of the last sub-slice of positive weight alone
    assert want["off"][-1] == want["off"][-2] and want["off"][1] == (ref["s"] == last).sum() > 0


def test_two_bunches(api):
    deck, beam, soa, want, ref, _ = _case(api, "two_bunches")
    lw = ref["table"]["lw"]
    assert (lw[13:18] == 0.0).all() and (lw[ref["s"]] > 0.0).all() and (ref["s"] < 12).any() and (ref["s"] > 18).any()
    assert not ((soa[2] > -0.2) & (soa[2] < 0.15)).any()      # (the sub-slices that hold z = -0.23 and 0.18 end there)


def test_pdf_positive_in_the_last_sub_slice_only(api):
    deck, beam, soa, want, ref, _ = _case(api, "last_sub_slice")
    assert (ref["s"] == 31).all() and want["off"][1] == 1000 and soa[2].min() >= 0.75 and soa[2].max() < 0.8


@pytest.mark.parametrize("ratio", [1, 3, 4])
def test_pdf_ref_ratio(api, ratio):
    deck, beam, soa, want, ref, _ = _case(api, {1: "ratio_1", 3: "ratio_3", 4: "gaussian"}[ratio])
    assert ref["table"]["ns"] == 8 * ratio and ref["s"].max() == 8 * ratio - 1


# ---- 2. the programs ----------------------------------------------------------------------------------------------------------

def test_every_program_is_bit_equal_at_the_devices_z(api):
    """A beam of means 0 and widths 1 with the same seed holds the device's own deviates (0 + 1 n = n exactly), at the same z and in
    the same order; with them every one of the ten programs shows bit for bit: x = X(z) + std_x(z) n_x, u_d = um_d(z) + us_d(z) m_d."""
    deck, beam, soa, want, ref, eng = _case(api, "programs")
    _, _, unit, _, _, _ = _case(api, "programs_unit")
    assert soa.shape[1] == 4096 and np.array_equal(soa[2], unit[2])
    z = soa[2]
    fn = [R.function(v, beam["constants"]) for k in ("position_mean", "position_std", "u_mean", "u_std") for v in beam[k]]
    assert [p.ins for p in eng.beam_pdf_programs[1]] == [f.__self__.ins for f in fn]
    assert np.array_equal(soa[0], fn[0](z) + fn[2](z) * unit[0]) and np.array_equal(soa[1], fn[1](z) + fn[3](z) * unit[1])
    for d in range(3):
        assert np.array_equal(soa[3 + d], fn[4 + d](z) + fn[7 + d](z) * unit[3 + d]), d
        assert np.ptp(fn[4 + d](z)) > 0 and np.ptp(fn[7 + d](z)) > 0
    assert (z > 0).any() and (z < 0).any()      # both arms of position_mean[1]'s if


# ---- 3. do_symmetrize, z_foc, the radius --------------------------------------------------------------------------------------

def test_symmetrized_beam(api):
    deck, beam, soa, want, ref, eng = _case(api, "symmetrized")
    assert beam["num_particles"] == 4096 and ref["z"].size == 1024
    assert (want["off"] % 4 == 0).all() and np.array_equal(want["i"][0::4], want["i"][3::4])
    q4 = soa.reshape(7, -1, 4)
    X, Y = ref["X"][want["i"][0::4]], ref["Y"][want["i"][0::4]]
    for q, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):      # the reference's order
        assert np.array_equal(q4[2, :, q], q4[2, :, 0]) and np.array_equal(q4[5, :, q], q4[5, :, 0])
        assert np.array_equal(q4[3, :, q], sx * q4[3, :, 0]) and np.array_equal(q4[4, :, q], sy * q4[4, :, 0])
        assert np.abs((q4[0, :, q] - X) - sx * (q4[0, :, 0] - X)).max() <= 4 * EPS * np.abs(q4[0]).max()
        assert np.abs((q4[1, :, q] - Y) - sy * (q4[1, :, 0] - Y)).max() <= 4 * EPS * np.abs(q4[1]).max()
    with pytest.raises(RuntimeError, match="num_particles must be divisible by 4"):
        eng.set_beam_fixed_weight_pdf(**dict(beam, num_particles=4098))


def test_z_foc(api):
    deck, beam, soa, want, ref, _ = _case(api, "focus")
    _, plain = _reference(api, deck, dict(beam, z_foc=0.0))
    assert np.array_equal(plain["off"], want["off"]) and np.array_equal(plain["soa"][2:], want["soa"][2:])
    assert np.abs(plain["soa"][0] - want["soa"][0]).max() > 1e-4


def test_density_with_a_radius_that_cuts(api):
    deck, beam, soa, want, ref, _ = _case(api, "radius_density")
    assert want["n_invalid"] > 1000 and want["n_outside"] == 0 and soa.shape[1] == 4096 - want["n_invalid"]
    draw = want["i"]
    assert ((soa[0] - ref["X"][draw]) ** 2 + (soa[1] - ref["Y"][draw]) ** 2 <= beam["radius"] ** 2 * (1 + 1e-9)).all()


def test_total_charge_with_a_radius_that_cuts(api):
    """nothing invalid and exactly num_particles kept; the attempt of every draw shows in its offsets: they are the restatement's
    pair of that attempt (to the bound), and the pairs of the other attempts lie far from them"""
    deck, beam, soa, want, ref, _ = _case(api, "si_charge")
    assert want["n_invalid"] == 0 and want["n_outside"] == 0 and soa.shape[1] == beam["num_particles"] == 1000
    assert ref["attempt"].max() >= 3 and (ref["attempt"] > 0).sum() > 200
    w = abs(beam["total_charge"] / deck["beam_charge"]) / beam["num_particles"]
    assert np.abs(soa[6] / w - 1.0).max() <= 4 * EPS
    first = R.fixed_weight_pdf_beam(deck, _pe_of(api, deck, beam), **dict(beam, radius=np.inf))      # every draw's first pair
    moved = ref["attempt"][want["i"]] > 0      # the first pair of these draws was refused: the device's offsets are another pair's
    dx = np.abs((soa[0] - ref["X"][want["i"]]) - first["x"][want["i"]])
    assert (dx[moved] > 1e-6 * beam["radius"]).all() and (dx[~moved] <= 1e-13 * ref["sx"][want["i"]][~moved]).all()


# ---- 4. no dependence on the launch -------------------------------------------------------------------------------------------

def test_draws_do_not_depend_on_the_number_of_particles(api):
    (deck, small), (_, large) = CASES["launch_4099"], CASES["launch_8198"]
    sa, wa, _, _ = _pair(api, deck, small)
    sb, wb, _, _ = _pair(api, deck, large)
    sub = wb["i"] < small["num_particles"]
    assert sub.sum() == sa.shape[1] == 4099 and sb.shape[1] == 8198
    assert np.array_equal(sa[:6], sb[:6, sub])
    wn_a, wn_b = sa[6] * small["num_particles"], sb[6, sub] * large["num_particles"]
    assert np.abs(wn_a - wn_b).max() <= 4 * EPS * wn_a.max()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_sizes(api, n):
    _case(api, f"size_{n}")


# ---- 5. refusals of the C entry point -----------------------------------------------------------------------------------------

def test_refusals_leave_the_engines_beam_in_place(api):
    deck, beam = CASES["gaussian"]
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_beam_fixed_weight_pdf(**dict(beam, num_particles=500))
    n, off = eng.beam_layout()
    _, soa = eng.beam_state()
    assert n == 500
    inf = np.inf
    for change, message in (
            (dict(pdf="z"), "PDF must be >= 0 everywhere"),
            (dict(pdf="1/(z-z)"), "PDF must be >= 0 everywhere"),
            (dict(pdf="0"), "the integral over the box must be positive"),
            (dict(pdf="z>5"), "the integral over the box must be positive"),
            (dict(position_std=(0.0, 0.25)), "position_std must be positive and finite"),
            (dict(position_std=(0.3, "z")), "position_std must be positive and finite"),
            (dict(density=None, total_charge=1.0e-12), "total_charge is only valid in SI units"),
            (dict(num_particles=0), "num_particles must be positive"),
            (dict(num_particles=4098, do_symmetrize=True), "num_particles must be divisible by 4"),
            (dict(num_particles=2 ** 32), "2\\^32 draws or more"),
            (dict(pdf_ref_ratio=0), "pdf_ref_ratio must be at least 1"),
            (dict(pdf_ref_ratio=2 ** 30), "overflows an int"),
            (dict(radius=0.0), "radius must be positive"),
            (dict(radius=-1.0), "radius must be positive"),
            (dict(z_foc=inf), "z_foc must be finite")):
        with pytest.raises(RuntimeError, match=message):
            eng.set_beam_fixed_weight_pdf(**dict(beam, **change))
        n1, off1 = eng.beam_layout()
        assert n1 == n and np.array_equal(off1, off) and np.array_equal(eng.beam_state()[1], soa), change      # refused ahead of any change
    assert sum(eng.set_beam_fixed_weight_pdf(**dict(beam, position_std=(0.3, "if(z>-0.9, 0.25, 0)")))) == 0      # zero only outside the box
    assert sum(eng.set_beam_fixed_weight_pdf(**dict(beam, radius=inf))) == 0 and eng.beam_layout()[0] == 4096
    n, off = eng.beam_layout()
    eng.run_step()
    with pytest.raises(RuntimeError, match="before the first hps_engine_begin_step"):
        eng.set_beam_fixed_weight_pdf(**beam)
    n1, off1 = eng.beam_layout()
    assert n1 == n and np.array_equal(off1, off)
    with pytest.raises(ValueError, match="beam_fixed_weight_pdf and beam_fixed_weight"):
        api.SliceEngine(dict(decks.with_fixed_weight_pdf_beam(deck, **beam), beam_fixed_weight=dict(num_particles=4)), tile_size=0)


# ---- 6. whole engines ---------------------------------------------------------------------------------------------------------

def _slices_as_sets(bnda, soaa, bndb, soab, nz, tol=1e-8):
    assert np.array_equal(bnda, bndb)
    scale = np.abs(soaa).max(axis=1, keepdims=True)
    for p in range(nz):
        sa, sb = soaa[:, bnda[p]:bnda[p + 1]], soab[:, bndb[p]:bndb[p + 1]]
        sa, sb = sa[:, np.lexsort(sa[::-1])], sb[:, np.lexsort(sb[::-1])]
        assert (np.abs(sa - sb) <= tol * scale).all(), p


def test_moving_beam(api):
    deck = dict(decks.beam_evolution(), n_steps=3)
    beam = R.MOVING_BEAM
    a = api.SliceEngine(decks.with_fixed_weight_pdf_beam(deck, **beam), tile_size=0)
    ref, want = _reference(api, deck, beam)
    assert a.deck["dt"] != 0.0 and a.beam_left_out == (want["n_invalid"], want["n_outside"]) and a.beam_left_out[0] > 0
    bnd0, soa0 = a.beam_state()
    n = soa0.shape[1]
    assert n + sum(a.beam_left_out) == beam["num_particles"] and n > 1500 and np.array_equal(bnd0, want["off"])
    b = api.SliceEngine(dict(deck, beam_profile=-1), tile_size=0)
    assert b.set_beam_particles(soa0) == 0
    for _ in range(2):
        a.run_step()
        b.run_step()
    bnda, soaa = a.beam_state()
    bndb, soab = b.beam_state()
    assert soaa.shape[1] == n and np.abs(soaa[:2] - soa0[:2]).max() > 1e-3      # conserved, and moved
    _slices_as_sets(bnda, soaa, bndb, soab, deck["nz"])


def test_transverse_benchmark_with_the_parsed_beam(api):
    deck = decks.transverse_benchmark(nxy=31, nz=40)
    beam = decks.TRANSVERSE_BENCHMARK_BEAM_PARSED(31)
    a = api.SliceEngine(decks.with_fixed_weight_pdf_beam(deck, **beam), tile_size=0)
    assert a.beam_left_out == (0, 0) and a.beam_layout()[0] == beam["num_particles"] == 9610
    assert abs(a.beam_uz_moments[0] - 2000.0) <= 160 * EPS * 2000.0      # (the 160 additions of the sum)
    ref, want = _reference(api, deck, beam)
    bnd0, soa0 = a.beam_state()
    assert np.array_equal(bnd0, want["off"]) and np.abs(soa0[2] - want["soa"][2]).max() <= 1e-13 * 12.0
    b = api.SliceEngine(deck, tile_size=0)
    assert b.set_beam_particles(soa0) == 0
    for e in (a, b):
        e.set_diagnostics(True)
        e.run_step()
    ca, cb = a.checksums(), b.checksums()
    assert ca["jz_beam"] != 0.0
    for k in ca:
        assert abs(ca[k] - cb[k]) <= 1e-8 * max(abs(cb[k]), 1e-300), (k, ca[k], cb[k])
    bnda, soaa = a.beam_state()
    bndb, soab = b.beam_state()
    _slices_as_sets(bnda, soaa, bndb, soab, deck["nz"])


# ---- 7. the prologue and the tail that the three device generators share --------------------------------------------------------

def _installed(eng):
    """what the engine holds of its beam: count, offsets, the beam as it is now (the moving beam's storage with hipace.dt != 0)
    and the injected blocks"""
    import torch
    n, off = eng.beam_layout()
    bnd, soa = eng.beam_state()
    blocks = torch.zeros(7 * max(n, 1), dtype=torch.float64, device="cuda")
    if n:
        eng.initial_beam_into(blocks)
    return n, off, bnd, soa, blocks.cpu().numpy()[:7 * n]


@pytest.mark.parametrize("dt", [0.0, 0.5])
def test_one_engine_takes_every_generator_in_turn(api, dt):
    """fixed_ppc, fixed_weight (257), fixed_weight_pdf (65), a fixed_weight beam whose zmin / zmax cut every draw away (n = 0) and
    fixed_ppc again on ONE engine: after every call the engine holds exactly what a fresh engine holds after the same call alone
    -- nothing of the beam before it is left in the offsets, the blocks, the moving beam's storage or the left-out counts.  The C
    ABI does not show the beam's box; for the static beam the step at the end deposits inside it on both engines (the deposited
    currents agree to 1e-9, the order of the atomic additions; a box of another beam would cut the current off)."""
    from tests import beam_fixed_weight_reference as F
    deck = dict(R.small_deck(), dt=dt, beam_ppc=(2, 2, 1), beam_radius=0.9, beam_pos_mean=(0.1, -0.1, 0.0), beam_zmin=-0.5,
                beam_zmax=0.7, beam_umean=(0.0, 0.0, 100.0))
    fw = dict(F.cases()["size_257"][1])
    steps = [("fixed_ppc", lambda e: e.set_beam_fixed_ppc("1 + 0.5*x", u_std=(0.2, 0.0, 1.0), random_ppc=(1, 0, 0), seed=3)),
             ("fixed_weight", lambda e: e.set_beam_fixed_weight(**fw)),
             ("fixed_weight_pdf", lambda e: e.set_beam_fixed_weight_pdf(**CASES["size_65"][1])),
             ("nothing", lambda e: e.set_beam_fixed_weight(**dict(fw, zmin=5.0, zmax=6.0)))]
    steps.append(steps[0])
    fresh = {}
    eng = api.SliceEngine(deck, tile_size=0)
    for name, call in steps:
        if name not in fresh:
            other = api.SliceEngine(deck, tile_size=0)
            fresh[name] = (call(other), _installed(other), other)
        left = call(eng)
        want_left, want, _ = fresh[name]
        got = _installed(eng)
        assert left == want_left, (name, left, want_left)
        assert got[0] == want[0], (name, got[0], want[0])
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(a, b), name
    assert fresh["fixed_ppc"][1][0] > 100 and fresh["fixed_weight"][0] != (0, 0) and 0 < fresh["fixed_weight"][1][0] < 257
    assert fresh["fixed_weight_pdf"][1][0] == 65 and fresh["nothing"][0] == (257, 0) and fresh["nothing"][1][0] == 0
    if dt == 0.0:
        other = fresh["fixed_ppc"][2]
        for e in (eng, other):
            e.set_diagnostics(True)
            e.run_step()
        ca, cb = eng.checksums(), other.checksums()
        assert cb["jz_beam"] != 0.0
        for k in ("jx_beam", "jy_beam", "jz_beam"):
            assert abs(ca[k] - cb[k]) <= 1e-9 * max(abs(cb[k]), 1e-300), (k, ca[k], cb[k])
