"""<beam>.do_salame without a GPU: the Python deck mirror against include/hpslice.h, the SALAME test decks, and the
pipeline's refusal (which must not touch a device)."""
import os
import re

import numpy as np
import pytest

from hipace_amd import _lib, decks, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FIELDS = ["beam_do_salame", "salame_n_iter", "salame_relative_tolerance", "salame_no_advance", "salame_Ez_target_slope"]


def _header_deck_fields():
    """the member names of hps_deck in include/hpslice.h, in order"""
    hdr = open(os.path.join(ROOT, "include", "hpslice.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = hdr[:hdr.index("} hps_deck;")].rsplit("typedef struct {", 1)[1]
    names = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        decl = re.sub(r"^(unsigned long long|double|int)\s+", "", stmt)
        for item in decl.split(","):
            names.append(re.match(r"\s*([A-Za-z_0-9]+)", item).group(1))
    return names


def test_deck_mirror_carries_the_salame_fields_in_header_order():
    hdr = _header_deck_fields()
    mirror = [n for n, _ in _lib.Deck._fields_]
    assert mirror == hdr
    assert hdr[-len(NEW_FIELDS):] == NEW_FIELDS                    # appended at the end, behind ext_Ez_slope
    assert hdr[-len(NEW_FIELDS) - 1] == "ext_Ez_slope"
    types = dict(_lib.Deck._fields_)
    import ctypes as C
    assert [types[n] for n in NEW_FIELDS] == [C.c_int, C.c_int, C.c_double, C.c_int, C.c_double]


def test_salame_defaults_are_zero_and_off():
    """0 = off / the reference's default (n_iter 5, tolerance 1e-4, do_advance on, slope 0); a deck without the keys has 0"""
    assert decks.SALAME_DEFAULT == dict(beam_do_salame=0, salame_n_iter=0, salame_relative_tolerance=0.0, salame_no_advance=0,
                                        salame_Ez_target_slope=0.0)
    dk = _lib.fill_struct(_lib.Deck(), decks.blowout_wake())
    assert [getattr(dk, n) for n in NEW_FIELDS] == [0, 0, 0.0, 0, 0.0]
    dk = _lib.fill_struct(_lib.Deck(), decks.salame_grid_current())
    assert [getattr(dk, n) for n in NEW_FIELDS] == [1, 0, 0.0, 0, 0.0]
    assert len(_lib.COMPS_SALAME) == 12


def test_salame_deck_is_what_the_issue_asks_for():
    d = decks.salame_grid_current()
    assert (d["nx"], d["ny"], d["nz"], d["order"], d["bxby_solver"]) == (64, 64, 100, 2, 0)
    assert tuple(d["plasma_ppc"]) == (2, 2) and d["mg_tol_rel"] == 1.0e-10 and d["dt"] == 0.0
    assert d["grid_current_on"] == 1 and d["grid_current_peak"] < 0.0 and 0.3 <= abs(d["grid_current_peak"]) <= 0.8
    assert d["beam_profile"] == 1 and tuple(d["beam_umean"][:2]) == (0.0, 0.0) and d["beam_umean"][2] > 0.0
    assert 2.0 <= d["beam_zmax"] - d["beam_zmin"] <= 3.0 and abs(d["beam_radius"] - 0.3) < 1e-12
    assert d["grid_current_mean"][2] > d["beam_zmax"]              # the driver is ahead of the witness
    o = decks.salame_grid_current_overload()
    assert o["beam_zmin"] < -2.0 < d["beam_zmin"]                  # past the sign change of the unloaded Ez at z = -2.0
    assert {k: v for k, v in o.items() if k != "beam_zmin"} == {k: v for k, v in d.items() if k != "beam_zmin"}


def test_si_twin_scales_all_lengths_by_one_factor():
    n, s = decks.salame_grid_current(), decks.salame_grid_current_SI()
    kp_inv = s["hi"][0] / n["hi"][0]
    assert kp_inv == pytest.approx(10.0e-6, rel=1e-15)
    for key in ("lo", "hi", "grid_current_mean", "grid_current_std"):
        np.testing.assert_allclose(s[key], np.asarray(n[key]) * kp_inv, rtol=1e-14, atol=0.0)
    for key in ("beam_zmin", "beam_zmax", "beam_radius"):
        assert s[key] == pytest.approx(n[key] * kp_inv, rel=1e-14)
    ne = s["plasma_density"]
    assert s["beam_density"] == pytest.approx(n["beam_density"] * ne, rel=1e-14)
    assert s["grid_current_peak"] == pytest.approx(n["grid_current_peak"] * ne * decks.SI["q_e"] * decks.SI["c"], rel=1e-14)
    # kp_inv is the skin depth of that density
    wp = (ne * decks.SI["q_e"] ** 2 / (decks.SI["m_e"] * decks.SI["ep0"])) ** 0.5
    assert decks.SI["c"] / wp == pytest.approx(kp_inv, rel=1e-12)
    same = ("nx", "ny", "nz", "order", "plasma_ppc", "beam_ppc", "beam_umean", "beam_profile", "mg_tol_rel", "beam_do_salame",
            "salame_n_iter", "salame_relative_tolerance", "salame_no_advance", "grid_current_on", "n_steps", "dt")
    assert all(s[k] == n[k] for k in same) and s["si_units"] == 1 and n["si_units"] == 0
    # the same particles land on the same slices
    dzn, dzs = (n["hi"][2] - n["lo"][2]) / n["nz"], (s["hi"][2] - s["lo"][2]) / s["nz"]
    zn = n["lo"][2] + (np.arange(n["nz"]) + 0.5) * dzn
    zs = s["lo"][2] + (np.arange(s["nz"]) + 0.5) * dzs
    inn = (zn < n["beam_zmax"]) & (zn >= n["beam_zmin"])
    ins = (zs < s["beam_zmax"]) & (zs >= s["beam_zmin"])
    assert (inn == ins).all() and np.flatnonzero(inn).tolist() == list(range(47, 63))


class _NoDevice:
    """stands where an engine would: any use beyond reading the deck fails the test"""

    def __init__(self, deck):
        self.deck = deck

    def __getattr__(self, name):
        raise AssertionError("the pipeline touched the engine (%s) before refusing the SALAME deck" % name)


def test_pipeline_refuses_a_salame_deck_without_touching_a_device():
    e = _NoDevice(decks.salame_grid_current())
    with pytest.raises(NotImplementedError, match="beam_do_salame"):
        pipeline.run_local_pipeline([e], 1, 0)
    with pytest.raises(NotImplementedError, match="beam_do_salame"):
        pipeline.run_lanes([e], 0, 1, 1, 0)
    with pytest.raises(NotImplementedError, match="beam_do_salame"):
        next(pipeline._stage(e, 0, 1, 1, 0))
    with pytest.raises(NotImplementedError, match="beam_do_salame"):
        pipeline.run_pipeline(e, 0, 1, 1, 0)
