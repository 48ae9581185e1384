"""The fixed_weight beam without a GPU: the numpy restatement (tests/beam_fixed_weight_reference.py) held to the margin condition
for every case of tests/test_beam_fixed_weight_gpu.py and to the moments of its parameters, the deck entry, the ABI and the
mean programs."""
import os
import re

import numpy as np
import pytest

from hipace_amd import _lib, decks, expr
from tests import beam_fixed_weight_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


def _run(name):
    deck, beam = CASES[name]
    return deck, beam, R.fixed_weight_beam(deck, **beam)


# ---- the margin condition -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_no_draw_of_a_gpu_case_lies_on_a_cut(name):
    """Then a last-bit difference in a transcendental cannot move a particle across a cut: counts and offsets compare exactly."""
    deck, beam, ref = _run(name)
    dt, dz, dr = R.margins(deck, ref, beam["position_std"], beam.get("zmin", -np.inf), beam.get("zmax", np.inf), beam.get("radius", np.inf))
    assert dt > 1e-9 and dz > 1e-9 and dr > 1e-9, (dt, dz, dr)


def test_gaussian_weight_deck_keeps_the_margin():
    deck = decks.with_fixed_weight_beam(*decks.gaussian_weight_SI(), seed=2)      # the GPU test's seed
    beam = decks.beam_fixed_weight(deck)
    ref = R.fixed_weight_beam(deck, **beam)
    dt, dz, dr = R.margins(deck, ref, beam["position_std"], beam["zmin"], beam["zmax"], beam["radius"])
    assert dt > 1e-9 and dz > 1e-9 and dr > 1e-9, (dt, dz, dr)


# ---- moments ------------------------------------------------------------------------------------------------------------------

def _within_5_standard_errors(v, mean, std):
    n = v.size
    assert abs(v.mean() - mean) <= 5.0 * std / np.sqrt(n), (v.mean(), mean)
    if std == 0.0:
        assert (v == mean).all()
    else:
        assert abs(v.std() - std) <= 5.0 * std / np.sqrt(2.0 * n), (v.std(), std)


def test_moments_of_the_gaussian_profile():
    deck = R.small_deck()
    beam = dict(num_particles=100000, position_mean=(0.11, "-0.07", 0.1), position_std=(0.3, 0.25, 0.5), u_mean=(1.0, -2.0, 100.0),
                u_std=(0.5, 0.0, 3.0), density=2.0, seed=21)
    ref = R.fixed_weight_beam(deck, **beam)
    assert ref["valid"].all()
    soa = ref["soa"]
    for r in range(3):
        _within_5_standard_errors(soa[r], float(beam["position_mean"][r]), beam["position_std"][r])
        _within_5_standard_errors(soa[3 + r], beam["u_mean"][r], beam["u_std"][r])
    for a, b in (("n_z", "n_x"), ("n_x", "n_y"), ("n_z", "n_y")):      # independent streams
        assert abs(np.mean(ref[a] * ref[b])) <= 5.0 / np.sqrt(100000)
    for d in range(3):
        assert abs(np.mean(ref["m"][d] * ref["n_x"])) <= 5.0 / np.sqrt(100000)


def test_moments_of_the_can_profile():
    deck = R.small_deck()
    beam = dict(num_particles=100000, position_mean=(0.0, 0.0, 5.0), position_std=(0.3, 0.25, 0.5), u_mean=(0.0, 0.0, 100.0),
                density=2.0, profile="can", zmin=-0.55, zmax=0.7, duz_per_uz0_dzeta=0.3, seed=22)
    ref = R.fixed_weight_beam(deck, **beam)
    z = ref["soa"][2]
    assert ref["valid"].all() and z.min() >= -0.55 and z.max() < 0.7
    _within_5_standard_errors(z, 0.075, 1.25 / np.sqrt(12.0))
    # the chirp is about (zmin + zmax) / 2 and leaves the mean alone
    assert np.array_equal(ref["soa"][5], 100.0 + (z - 0.5 * (-0.55 + 0.7)) * 0.3 * 100.0)
    assert abs(ref["soa"][5].mean() - 100.0) <= 5.0 * 30.0 * 1.25 / np.sqrt(12.0) / np.sqrt(100000)


@pytest.mark.parametrize("si", [False, True])
def test_weight_sum_is_the_closed_form(si):
    deck = R.small_deck(si=si)
    u = 10.0e-6 if si else 1.0
    std = (0.3 * u, 0.25 * u, 0.05 * u)      # nothing outside the box
    n, n0 = 1000, 2.0e20 if si else 2.0
    ref = R.fixed_weight_beam(deck, num_particles=n, position_mean=(0.0, 0.0, 0.0), position_std=std, density=n0, seed=23)
    got = R.binned(deck, ref)
    assert got["n_outside"] == 0 and got["n_invalid"] == 0 and got["soa"].shape[1] == n
    h = R.cell_size(deck)
    want = n0 * (2.0 * np.pi) ** 1.5 * std[0] * std[1] * std[2] / (1.0 if si else h[0] * h[1] * h[2])
    assert abs(got["soa"][6].sum() - want) <= (R.WEIGHT_ROUNDINGS + n) * np.finfo(float).eps * want
    q = deck["beam_charge"]
    by_charge = R.weight(deck, n, std, total_charge=want * q) if si else None
    assert by_charge is None or abs(by_charge * n - want) <= 4 * np.finfo(float).eps * want


def test_symmetrized_copies_mirror_exactly():
    deck, beam, ref = _run("symmetrized")
    q4 = ref["soa"].reshape(7, -1, 4)
    assert q4.shape[1] == beam["num_particles"] // 4
    for q, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
        assert np.array_equal(q4[0, :, q], ref["X"] + ref["x"] if sx > 0 else ref["X"] - ref["x"])      # (no z_foc in this case)
        assert np.array_equal(q4[1, :, q], ref["Y"] + ref["y"] if sy > 0 else ref["Y"] - ref["y"])
        assert np.array_equal(q4[3, :, q], sx * q4[3, :, 0]) and np.array_equal(q4[4, :, q], sy * q4[4, :, 0])
        for r in (2, 5, 6):
            assert np.array_equal(q4[r, :, q], q4[r, :, 0])
    assert np.array_equal(ref["valid"].reshape(-1, 4).all(axis=1), ref["valid"].reshape(-1, 4).any(axis=1))


def test_draws_do_not_depend_on_the_number_of_particles():
    (deck, small), (_, large) = CASES["launch_4099"], CASES["launch_8198"]
    a, b = R.fixed_weight_beam(deck, **small), R.fixed_weight_beam(deck, **large)
    n = small["num_particles"]
    assert np.array_equal(a["soa"][:6], b["soa"][:6, :n]) and np.array_equal(a["valid"], b["valid"][:n])
    c = R.fixed_weight_beam(deck, **dict(small, num_particles=99), first=4000)
    assert np.array_equal(c["soa"][:6], a["soa"][:6, 4000:])
    assert not np.array_equal(R.fixed_weight_beam(deck, **dict(small, seed=7))["z"], a["z"])


# ---- the deck -----------------------------------------------------------------------------------------------------------------

def test_deck_entry_is_kept_apart_from_the_pinned_groups():
    keys = set(decks.BEAM_FIXED_WEIGHT_DEFAULT)
    assert "beam_fixed_weight" not in decks._DEFAULT and "beam_fixed_weight" not in decks.BEAM_INIT_DEFAULT
    fields = {n for n, _ in _lib.Deck._fields_}
    assert "beam_fixed_weight" not in fields and not keys & fields and not keys & set(decks.BEAM_INIT_DEFAULT) and not keys & set(decks._DEFAULT)
    for make in (decks.blowout_wake, decks.linear_wake, decks.beam_evolution, decks.adaptive_time_step, decks.blowout_wake_SI,
                 lambda: decks.gaussian_weight_SI()[0], lambda: decks.hosing()[0]):
        assert "beam_fixed_weight" not in make() and decks.beam_fixed_weight(make()) is None
    assert decks.BEAM_FIXED_WEIGHT_DEFAULT["profile"] == "gaussian" and decks.BEAM_FIXED_WEIGHT_DEFAULT["seed"] == 1


def test_with_fixed_weight_beam_carries_the_files_parameters():
    base, beam = decks.gaussian_weight_SI()
    d = decks.with_fixed_weight_beam(*decks.gaussian_weight_SI())
    assert {k: v for k, v in d.items() if k != "beam_fixed_weight"} == base and "beam_fixed_weight" not in base
    spec = decks.beam_fixed_weight(d)
    assert set(spec) == set(decks.BEAM_FIXED_WEIGHT_DEFAULT)
    assert spec["num_particles"] == 100000 and spec["total_charge"] == 1.0e-9 and spec["density"] is None
    assert spec["position_mean"] == (0.0, 10.0e-6, 20.0e-6) and spec["position_std"] == (30.0e-6, 40.0e-6, 50.0e-6)
    assert spec["u_mean"] == (0.0, 0.0, 1.0e3) and (spec["zmin"], spec["zmax"], spec["radius"]) == (-1.0, 1.0, 1.0)
    assert spec["profile"] == "gaussian" and spec["seed"] == 1 and not spec["do_symmetrize"]
    assert decks.beam_fixed_weight(decks.with_fixed_weight_beam(base, beam, seed=5, do_symmetrize=True))["seed"] == 5
    rr = decks.beam_fixed_weight(decks.with_fixed_weight_beam(*decks.radiation_reaction_SI()))
    assert rr["u_std"][1] == 0.0 and rr["u_std"][0] > 0.0 and rr["density"] == 5.0e24 / 1.0e10
    with pytest.raises(ValueError, match="Python callable"):
        decks.with_fixed_weight_beam(*decks.hosing())
    with pytest.raises(ValueError, match="unknown beam parameter 'ppc'"):
        decks.with_fixed_weight_beam(base, beam, ppc=(1, 1, 1))
    with pytest.raises(ValueError, match="unknown entries"):
        decks.beam_fixed_weight(dict(base, beam_fixed_weight=dict(number=3)))
    with pytest.raises(ValueError, match="beam_fixed_weight and beam_density_expr"):
        decks.beam_fixed_weight(dict(d, beam_density_expr="1"))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_header_signature_table_and_makefile():
    hdr = open(os.path.join(ROOT, "include", "hpslice.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+hps_engine_set_beam_fixed_weight\s*\(([^)]*)\)", code)
    assert m and len(m.group(1).split(",")) == 6
    assert re.search(r"\}\s*hps_beam_fixed_weight\s*;", code)
    assert "BeamParticleContainerInit.cpp:348-475" in hdr and "BeamParticleContainer.cpp:137-198" in hdr and "GetInitialMomentum.H:36-48" in hdr
    res, args = _lib._SIGS["hps_engine_set_beam_fixed_weight"]
    assert len(args) == 6
    struct = re.search(r"typedef struct \{([^}]*)\}\s*hps_beam_fixed_weight", code).group(1)
    names = re.findall(r"(\w+)(?:\[3\])?\s*[,;]", struct)
    assert names == [n for n, _ in _lib.BeamFixedWeight._fields_]
    mk = open(os.path.join(ROOT, "hipace_amd", "csrc", "Makefile")).read()
    assert "beam_init.hip" in mk
    src = open(os.path.join(ROOT, "hipace_amd", "csrc", "beam_init.hip")).read()
    assert "hps_engine_set_beam_fixed_weight" in src and "k_fw_fill" in src


# ---- the mean programs --------------------------------------------------------------------------------------------------------

def test_mean_programs_compile_over_z():
    _, beam = CASES["programs"]
    z = np.linspace(-0.8, 0.8, 33)
    px, py = (expr.compile_expr(beam["position_mean"][q], ("z",), beam["constants"]) for q in range(2))
    assert px.variables == ("z",) and np.allclose(px.evaluate(z), 0.2 * (z - 0.1), rtol=0, atol=1e-16)
    assert np.array_equal(py.evaluate(z), np.where(z > 0, 0.1, -0.1) + 0.05 * (z * z))
    assert expr.compile_expr(0.25, ("z",)).evaluate(z).tolist() == [0.25] * 33      # a number is a constant program
    for text in ("0.1*x", "z + t", "y"):
        with pytest.raises(ValueError, match="unknown name"):
            expr.compile_expr(text, ("z",))
