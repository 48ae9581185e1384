"""The fixed_weight_pdf beam without a GPU: the numpy restatement (tests/beam_fixed_weight_pdf_reference.py) held to the
distribution it stands for, to the host path's chain and the reference's formulae, and to the margin condition for every case of
tests/test_beam_fixed_weight_pdf_gpu.py; the deck entry, the ABI and Python's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from hipace_amd import _lib, api, decks
from tests import beam_fixed_weight_pdf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()
EPS = np.finfo(np.float64).eps


def _pe(deck, beam):
    """the pdf at the edges from the library's own host routine (hps_expr_eval_host: no device)"""
    return api.Expression(beam["pdf"], ("z",), beam.get("constants")).evaluate_host(R.edges(deck, beam.get("pdf_ref_ratio", 4)))


def _run(name, **change):
    deck, beam = CASES[name]
    beam = dict(beam, **change)
    return deck, beam, R.fixed_weight_pdf_beam(deck, _pe(deck, beam), **beam)


# ---- the margin condition -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_no_draw_of_a_gpu_case_lies_on_a_cut(name):
    """|t - cum[s]| over cum[ns], the slice coordinate's distance from an integer and |x^2 + y^2 - radius^2| over radius^2 (every
    attempt) all exceed 1e-9: a last-bit difference cannot move a draw across a cut, so counts and offsets compare exactly."""
    deck, beam, ref = _run(name)
    dt, dq, dr = R.margins(deck, ref)
    assert dt > 1e-9 and dq > 1e-9 and dr > 1e-9, (dt, dq, dr)
    assert (ref["table"]["lw"][ref["s"]] > 0.0).all()      # no draw lands in a sub-slice of zero weight


def test_whole_engine_cases_keep_the_margin():
    for deck, beam in ((decks.beam_evolution(), R.MOVING_BEAM), (decks.transverse_benchmark(nxy=31, nz=40), decks.TRANSVERSE_BENCHMARK_BEAM_PARSED(31))):
        ref = R.fixed_weight_pdf_beam(deck, _pe(deck, beam), **beam)
        dt, dq, dr = R.margins(deck, ref)
        assert dt > 1e-9 and dq > 1e-9 and dr > 1e-9, (dt, dq, dr)


# ---- the distribution ---------------------------------------------------------------------------------------------------------

def test_counts_per_sub_slice_follow_the_table():
    """Pearson's chi-square of the counts of 10^5 draws against N lw / integral over the 32 sub-slices of the gaussian case (the
    smallest expectation is 64 draws): 31 degrees of freedom, whose 0.999 quantile is 61.098.  Seed 1 is the only one tried."""
    deck, beam, ref = _run("gaussian", num_particles=100000)
    tab = ref["table"]
    expect = beam["num_particles"] * tab["lw"] / tab["integral"]
    assert tab["ns"] == 32 and expect.min() > 50.0
    counts = np.bincount(ref["s"], minlength=tab["ns"])
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"chi-square {chi2:.2f} for 31 degrees of freedom")
    assert chi2 < 61.098
    # the multinomial draw: sums exactly, whatever the table
    assert counts.sum() == beam["num_particles"]


def test_z_inside_a_sub_slice_follows_the_linear_profile():
    """The profile lo + (hi - lo) f on f in [0, 1] has the distribution function F(f) = (lo f + (hi - lo) f^2 / 2) / ((lo + hi) / 2).
    The square-root branch is its inverse (to rounding: 1e-12); the Taylor branch is the inverse to first order in
    d = (hi - lo)/(hi + lo): with lo = (1 - d) M, hi = (1 + d) M the equation is f = w + d f (1 - f), whose second-order term is
    d^2 w (1 - w)(1 - 2 w), at most 0.097 d^2 -- so the two differ by less than 0.2 d^2 where both apply (d < 1/21), and
    F(Taylor) misses w by less than (1 + d) 0.2 d^2."""
    w = np.linspace(0.0, 1.0, 2001)[:-1]
    def cdf(f, lo, hi):
        return (lo * f + 0.5 * (hi - lo) * f * f) / (0.5 * (lo + hi))
    for lo, hi in ((0.0, 1.0), (1.0, 0.0), (1.0, 3.0), (2.5, 0.3), (1.0, 1.2), (1.2, 1.0)):      # the square-root branch
        f, taylor = R.z_fraction(w, np.full_like(w, lo), np.full_like(w, hi))
        assert not taylor.any() and f.min() >= 0.0 and f.max() < 1.0 and (np.diff(f) > 0).all()
        assert np.abs(cdf(f, lo, hi) - w).max() <= 1e-12
    for lo, hi in ((1.0, 1.0), (1.0, 1.05), (1.05, 1.0), (3.0, 3.29), (3.29, 3.0)):      # the Taylor branch
        d = (hi - lo) / (hi + lo)
        f, taylor = R.z_fraction(w, np.full_like(w, lo), np.full_like(w, hi))
        assert taylor.all() and f.min() >= 0.0 and f.max() < 1.0 and (np.diff(f) > 0).all()
        assert np.abs(cdf(f, lo, hi) - w).max() <= (1.0 + abs(d)) * 0.2 * d * d + 4 * EPS
        with np.errstate(divide="ignore", invalid="ignore"):
            root = (np.sqrt(lo * lo + w * (hi * hi - lo * lo)) - lo) / (hi - lo) if hi != lo else w
        assert np.abs(f - root).max() <= 0.2 * d * d + 1e-12
    f, _ = R.z_fraction(w, np.full_like(w, 2.0), np.full_like(w, 2.0))
    assert np.array_equal(f, w)      # a constant pdf: z is uniform, bit for bit


def test_draws_inside_the_sub_slices_are_uniform_in_w():
    """the restatement's z, mapped back through F of its sub-slice, is the unit draw w: Kolmogorov-Smirnov distance of 10^5 draws
    against the uniform distribution below 1.95 / sqrt(N), the 0.001 point of the Kolmogorov distribution"""
    deck, beam, ref = _run("windowed", num_particles=100000)
    pe, tab = _pe(deck, beam), ref["table"]
    lo, hi = pe[ref["s"]], pe[ref["s"] + 1]
    f = (ref["z"] - (deck["lo"][2] + ref["s"] * tab["zs"])) / tab["zs"]
    assert f.min() >= 0.0 and f.max() <= 1.0
    F = np.sort((lo * f + 0.5 * (hi - lo) * f * f) / (0.5 * (lo + hi)))
    n = F.size
    ks = max(np.abs(F - np.arange(n) / n).max(), np.abs(F - np.arange(1, n + 1) / n).max())
    # (the Taylor branch's own deviation, 0.2 d^2 < 5e-4, lies below the bound's 6.2e-3)
    assert ks < 1.95 / np.sqrt(n), ks


# ---- the weight and the moments -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("si", [False, True])
def test_weight_equals_the_host_paths_chain_and_the_formula(si):
    deck = R.small_deck(si=si)
    u = 10.0e-6 if si else 1.0
    beam = dict(num_particles=1000, pdf=f"exp(-0.5*((z-{0.1 * u!r})/{0.3 * u!r})^2)", position_mean=(0.0, 0.0), position_std=(0.3 * u, 0.25 * u),
                u_mean=(0.0, 0.0, 100.0), density=2.0e20 if si else 2.0, seed=3)
    pe = _pe(deck, beam)
    ref = R.fixed_weight_pdf_beam(deck, pe, **beam)
    tab = ref["table"]
    bound = R.weight_roundings(tab["ns"]) * EPS
    host = decks.fixed_weight_pdf_beam(deck, beam["num_particles"], beam["density"], lambda z: pe, pos_std=beam["position_std"])
    assert np.abs(host[6] / tab["weight"] - 1.0).max() <= bound
    h = R.cell_size(deck)
    lw = 0.5 * (pe[:-1] + pe[1:])
    peak = lw.max() / (tab["zs"] * beam["position_std"][0] * beam["position_std"][1] * 2.0 * np.pi)
    want = beam["density"] * lw.sum() / peak / beam["num_particles"] / (1.0 if si else h[0] * h[1] * h[2])
    assert abs(tab["weight"] / want - 1.0) <= bound and (ref["soa"][6] == tab["weight"]).all()
    # the peak of the beam's density is `density`: weight N lw_max / integral particles in the fullest sub-slice's volume
    n_peak = tab["weight"] * beam["num_particles"] * lw.max() / lw.sum() * (1.0 if si else h[0] * h[1] * h[2])
    assert abs(n_peak / (tab["zs"] * 2.0 * np.pi * beam["position_std"][0] * beam["position_std"][1]) / beam["density"] - 1.0) <= bound
    if si:
        by_charge = R.fixed_weight_pdf_beam(deck, pe, **dict(beam, density=None, total_charge=3.0e-12))
        assert abs(by_charge["weight"] / (3.0e-12 / abs(deck["beam_charge"]) / 1000) - 1.0) <= 4 * EPS


def test_uz_moments_are_the_pdf_weighted_ones():
    deck, beam, ref = _run("gaussian")
    tab, pe = ref["table"], _pe(deck, beam)
    e = R.edges(deck)
    zmid, lw = 0.5 * (e[:-1] + e[1:]), 0.5 * (pe[:-1] + pe[1:])
    um, us = 100.0 + 20.0 * zmid, 3.0
    mean = np.average(um, weights=lw)
    std = np.sqrt(np.average(um * um + us * us, weights=lw) - mean * mean)
    assert abs(tab["uz_mean"] - mean) <= 1e-13 * mean and abs(tab["uz_std"] - std) <= 1e-10 * std and std > 3.0
    # ... and the draws' own moments, within 5 standard errors
    uz = ref["soa"][5]
    assert abs(uz.mean() - mean) <= 5.0 * std / np.sqrt(uz.size) and abs(uz.std() - std) <= 5.0 * std / np.sqrt(2.0 * uz.size)
    flat = R.table(deck, pe, 10, (0.3, 0.3), 2000.0, 0.0, density=1.0)
    # a beam without a spread: the difference under the root is a rounding of either sign about zero (ns roundings in each of the
    # two sums), and one below zero counts as zero -- never a NaN
    assert abs(flat["uz_mean"] - 2000.0) <= 32 * EPS * 2000.0 and 0.0 <= flat["uz_std"] <= 2000.0 * np.sqrt(4 * 32 * EPS)


def test_draws_do_not_depend_on_the_number_of_particles():
    (deck, small), (_, large) = CASES["launch_4099"], CASES["launch_8198"]
    pe = _pe(deck, small)
    a, b = R.fixed_weight_pdf_beam(deck, pe, **small), R.fixed_weight_pdf_beam(deck, pe, **large)
    n = small["num_particles"]
    assert np.array_equal(a["soa"][:6], b["soa"][:6, :n]) and np.array_equal(a["s"], b["s"][:n])
    c = R.fixed_weight_pdf_beam(deck, pe, **dict(small, num_particles=99), first=4000)
    assert np.array_equal(c["soa"][:6], a["soa"][:6, 4000:])
    assert not np.array_equal(R.fixed_weight_pdf_beam(deck, pe, **dict(small, seed=7))["z"], a["z"])


def test_symmetrized_copies_mirror_exactly():
    deck, beam, ref = _run("symmetrized")
    q4 = ref["soa"].reshape(7, -1, 4)
    assert q4.shape[1] == beam["num_particles"] // 4
    for q, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
        assert np.array_equal(q4[0, :, q], ref["X"] + ref["x"] if sx > 0 else ref["X"] - ref["x"])
        assert np.array_equal(q4[1, :, q], ref["Y"] + ref["y"] if sy > 0 else ref["Y"] - ref["y"])
        assert np.array_equal(q4[3, :, q], sx * q4[3, :, 0]) and np.array_equal(q4[4, :, q], sy * q4[4, :, 0])
        for r in (2, 5, 6):
            assert np.array_equal(q4[r, :, q], q4[r, :, 0])


def test_total_charge_redraws_until_inside_the_radius():
    deck, beam, ref = _run("si_charge")
    assert ref["valid"].all() and ref["attempt"].max() >= 3 and (ref["attempt"] == 0).sum() < 800
    assert (ref["x"] ** 2 + ref["y"] ** 2 <= beam["radius"] ** 2).all()
    deck, beam, ref = _run("radius_density")
    assert not ref["attempt"].any() and 1000 < (~ref["valid"]).sum() < 2000


# ---- the deck -----------------------------------------------------------------------------------------------------------------

def test_deck_entry_is_kept_apart_from_the_pinned_groups():
    keys = set(decks.BEAM_FIXED_WEIGHT_PDF_DEFAULT)
    name = "beam_fixed_weight_pdf"
    assert name not in decks._DEFAULT and name not in decks.BEAM_INIT_DEFAULT and name not in decks.BEAM_FIXED_WEIGHT_DEFAULT
    fields = {n for n, _ in _lib.Deck._fields_}
    assert name not in fields and not keys & fields and not keys & set(decks.BEAM_INIT_DEFAULT) and not keys & set(decks._DEFAULT)
    for make in (decks.blowout_wake, decks.linear_wake, decks.beam_evolution, decks.adaptive_time_step, decks.blowout_wake_SI,
                 decks.transverse_benchmark, lambda: decks.gaussian_weight_SI()[0], lambda: decks.hosing()[0],
                 lambda: decks.with_fixed_weight_beam(*decks.gaussian_weight_SI())):
        assert name not in make() and decks.beam_fixed_weight_pdf(make()) is None
    assert decks.BEAM_FIXED_WEIGHT_PDF_DEFAULT["pdf_ref_ratio"] == 4 and decks.BEAM_FIXED_WEIGHT_PDF_DEFAULT["seed"] == 1


def test_with_fixed_weight_pdf_beam_and_the_benchmark_beams():
    base = decks.transverse_benchmark(nxy=31, nz=40)
    parsed = decks.TRANSVERSE_BENCHMARK_BEAM_PARSED(31)
    d = decks.with_fixed_weight_pdf_beam(base, **parsed)
    assert {k: v for k, v in d.items() if k != "beam_fixed_weight_pdf"} == base and "beam_fixed_weight_pdf" not in base
    spec = decks.beam_fixed_weight_pdf(d)
    assert set(spec) == set(decks.BEAM_FIXED_WEIGHT_PDF_DEFAULT)
    host = decks.TRANSVERSE_BENCHMARK_BEAM(31)
    assert spec["num_particles"] == host["num_particles"] == 9610 and spec["density"] == host["density"] and spec["pdf"] == "exp(-0.5*(z/1.41)^2)"
    assert tuple(spec["position_std"]) == tuple(host["pos_std"]) and tuple(spec["u_mean"]) == tuple(host["u_mean"])
    z = R.edges(base)
    assert np.allclose(api.Expression(spec["pdf"], ("z",)).evaluate_host(z), host["pdf"](z), rtol=1e-15, atol=0)
    assert decks.beam_fixed_weight_pdf(decks.with_fixed_weight_pdf_beam(base, **dict(parsed, pos_std=(0.2, 0.1))))["position_std"] == (0.2, 0.1)
    with pytest.raises(ValueError, match="Python callable"):
        decks.with_fixed_weight_pdf_beam(base, **dict(parsed, pdf=host["pdf"]))
    with pytest.raises(ValueError, match="unknown beam parameter 'zmin'"):
        decks.with_fixed_weight_pdf_beam(base, **dict(parsed, zmin=0.0))
    with pytest.raises(ValueError, match="unknown entries"):
        decks.beam_fixed_weight_pdf(dict(base, beam_fixed_weight_pdf=dict(number=3)))
    with pytest.raises(ValueError, match="beam_fixed_weight_pdf and beam_density_expr"):
        decks.beam_fixed_weight_pdf(dict(d, beam_density_expr="1"))
    with pytest.raises(ValueError, match="beam_fixed_weight_pdf and beam_fixed_weight"):
        decks.beam_fixed_weight_pdf(dict(d, beam_fixed_weight=dict(num_particles=4)))
    # the timestep benchmark's proton driver: the window closes the pdf at both ends of the file's box
    ts = decks.timestep_benchmark_beam(num_particles=1000)
    assert ts["num_particles"] == 1000 and decks.timestep_benchmark_beam()["num_particles"] == 268 * 10 ** 9
    pdf = api.Expression(ts["pdf"], ("z",), ts["constants"])
    kp = np.sqrt(9.38e20 * decks.SI["q_e"] ** 2 / (decks.SI["m_e"] * decks.SI["ep0"])) / decks.SI["c"]
    zhi = 4 * 0.049 * kp
    v = pdf.evaluate_host(np.array([-1.01 * zhi, -0.99 * zhi, 0.0, 0.99 * zhi, 1.01 * zhi]))
    assert v[0] == 0.0 and v[4] == 0.0 and v[2] == 1.0 and abs(v[1] - np.exp(-0.5 * 3.96 ** 2)) <= 1e-12 and v[1] == v[3]
    sx = api.Expression(ts["position_std"][0], ("z",), ts["constants"]).evaluate_host(np.zeros(1))[0]
    assert abs(sx / (0.45e-3 * kp) - 1.0) <= 1e-14
    assert set(ts) <= set(decks.BEAM_FIXED_WEIGHT_PDF_DEFAULT)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_header_signature_table_and_struct():
    hdr = open(os.path.join(ROOT, "include", "hpslice.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+hps_engine_set_beam_fixed_weight_pdf\s*\(([^)]*)\)", code)
    assert m and len(m.group(1).split(",")) == 7
    assert "BeamParticleContainerInit.cpp:477-695" in hdr and "BeamParticleContainer.cpp:200-240" in hdr
    assert "position_mean x, position_mean y, position_std x, position_std y, u_mean x y z, u_std x y z" in hdr      # the order of progs
    res, args = _lib._SIGS["hps_engine_set_beam_fixed_weight_pdf"]
    assert len(args) == 7 and res is ctypes.c_int
    struct = re.search(r"typedef struct \{([^}]*)\}\s*hps_beam_fixed_weight_pdf\s*;", code).group(1)
    names = re.findall(r"(\w+)\s*[,;]", struct)
    assert names == [n for n, _ in _lib.BeamFixedWeightPdf._fields_]
    assert ctypes.sizeof(_lib.BeamFixedWeightPdf) == 56      # long, 2 int, 4 double, int, padding
    src = open(os.path.join(ROOT, "hipace_amd", "csrc", "beam_init.hip")).read()
    assert "hps_engine_set_beam_fixed_weight_pdf" in src and "k_fwp_keys" in src and "k_fwp_fill" in src
    assert re.search(r"BI_TAG_FW_PDF_Z\s*=\s*4\b", src) and R.TAG_PDF_Z == 4
    assert hasattr(_lib.lib(), "hps_engine_set_beam_fixed_weight_pdf")


# ---- Python's refusals (ahead of the engine: no device) -----------------------------------------------------------------------

def test_python_refusals():
    _, beam = CASES["gaussian"]
    call = api.SliceEngine.set_beam_fixed_weight_pdf
    for change, message in ((dict(total_charge=1.0), "exclusively either total_charge or density"),
                            (dict(density=None), "exclusively either total_charge or density"),
                            (dict(pdf="exp(-x*x)"), "pdf is a function of z alone"),
                            (dict(position_mean=("0.1*x", 0.0)), r"position_mean\[0\] is a function of z alone"),
                            (dict(position_std=(0.3, "0.1+t")), r"position_std\[1\] is a function of z alone"),
                            (dict(u_mean=(0.0, 0.0, "y")), r"u_mean\[2\] is a function of z alone"),
                            (dict(u_std=("z+k", 0.0, 0.0)), r"u_std\[0\] is a function of z alone"),
                            (dict(density="2*n0"), "density is a number"),
                            (dict(position_mean=(0.0, 0.0, 0.1)), "two entries each")):
        with pytest.raises(ValueError, match=message):
            call(None, **dict(beam, **change))
    with pytest.raises(TypeError):
        call(None, **dict(beam, zmin=0.0))
