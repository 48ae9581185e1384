"""SALAME on a witness species of a moving-beam engine, without a GPU: the deck plumbing, the ctypes mirrors against
include/hpslice.h, the pipeline's refusals (which must not touch a device) and the numpy restatements the GPU tests compare with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hipace_amd import _lib, decks, pipeline
from tests import beam_species_reference as S
from tests import external_field_reference as R
from tests import salame_moving_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpslice.h")).read(), flags=re.S)


def _struct_members(hdr, name):
    """the members of `typedef struct { ... } name;` in order -> [(C type, member)]"""
    body = hdr[:hdr.index("} " + name + ";")].rsplit("typedef struct {", 1)[1]
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        m = re.match(r"^(unsigned long long|unsigned char|double|long|int)\s+(.*)$", stmt, flags=re.S)
        for item in m.group(2).split(","):
            out.append((m.group(1), re.match(r"\s*([A-Za-z_0-9]+)", item).group(1)))
    return out


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_beam_species_mirror_follows_the_header_with_do_salame_last():
    members = _struct_members(_header(), "hps_beam_species")
    ctype = {"double": C.c_double, "int": C.c_int}
    assert [(n, t) for n, t in _lib.BeamSpecies._fields_] == [(n, ctype[t]) for t, n in members]
    assert members[-1] == ("int", "do_salame") and members[-2] == ("double", "uz_std")


def test_the_deck_struct_gains_no_member():
    """beam_species_salame is applied through a setter, as the collisions and the species themselves are: hps_deck and its
    mirror end with the members of <beam>.do_salame"""
    members = [n for _, n in _struct_members(_header(), "hps_deck")]
    assert members == [n for n, _ in _lib.Deck._fields_]
    assert members[-1] == "salame_Ez_target_slope" and "beam_species_salame" not in members
    assert "beam_species_salame" not in decks.SALAME_DEFAULT and decks.SALAME_SPECIES_DEFAULT == dict(beam_species_salame=0)


def test_header_declares_the_new_entry_points_and_lib_carries_them():
    hdr = _header()
    sigs = {"hps_engine_set_beam_species_salame": [C.c_void_p, C.c_int],
            "hps_engine_deposit_beam_species": [C.c_void_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int],
            "hps_engine_salame_scale_slice": [C.c_void_p, C.c_int, C.c_double]}
    ctype = {"void*": C.c_void_p, "int": C.c_int, "unsigned": C.c_uint, "double": C.c_double}
    for name, args in sigs.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, name
        declared = [ctype[re.sub(r"\s*[A-Za-z_0-9]+$", "", a.strip()).replace(" ", "")] for a in m.group(1).split(",")]
        assert declared == args, name
        assert _lib._SIGS[name] == (C.c_int, args), name
    lib = _lib.lib()
    for name in sigs:
        assert getattr(lib, name) is not None


# ---- the deck plumbing ----------------------------------------------------------------------------------------------------------
def test_do_salame_enters_the_record_only_where_the_entry_sets_it():
    deck = R.vacuum_deck()
    soa = np.zeros((7, 3))
    plain = decks.beam_species_spec(deck, dict(particles=soa, charge=1.0))
    assert "do_salame" not in plain["record"]
    assert _lib.fill_struct(_lib.BeamSpecies(), plain["record"]).do_salame == 0
    on = decks.beam_species_spec(deck, dict(particles=soa, charge=1.0, do_salame=1))
    assert on["record"]["do_salame"] == 1 and _lib.fill_struct(_lib.BeamSpecies(), on["record"]).do_salame == 1
    assert {k: v for k, v in on["record"].items() if k != "do_salame"} == plain["record"]
    off = decks.beam_species_spec(deck, dict(particles=soa, charge=1.0, do_salame=False))
    assert off["record"]["do_salame"] == 0
    assert decks.BEAM_SPECIES_DEFAULT["do_salame"] is None
    with pytest.raises(ValueError, match="unknown entries \\['do_salami'\\]"):
        decks.beam_species_spec(deck, dict(particles=soa, do_salami=1))


def test_beam_species_salame_is_derived_from_the_entries():
    deck = R.vacuum_deck()
    soa = np.zeros((7, 3))
    assert decks.beam_species_salame(deck) == 0
    assert decks.beam_species_salame(dict(deck, beam_species=[dict(particles=soa)])) == 0
    assert decks.beam_species_salame(dict(deck, beam_species=[dict(particles=soa), dict(particles=soa, do_salame=1)])) == 1
    assert decks.beam_species_salame(dict(deck, beam_species_salame=1)) == 1
    assert decks.beam_species_salame(dict(deck, beam_species_salame=0, beam_species=[dict(particles=soa, do_salame=0)])) == 0


def test_the_moving_decks_are_what_the_issue_asks_for():
    s, m = decks.salame_grid_current(), decks.salame_grid_current_moving()
    assert m["beam_profile"] == -1 and m["beam_do_salame"] == 0 and m["beam_species_salame"] == 1 and m["dt"] != 0.0
    changed = {"beam_profile", "beam_do_salame", "beam_species_salame", "dt", "beam_name", "beam_species"}
    assert {k: v for k, v in m.items() if k not in changed} == {k: v for k, v in s.items() if k not in changed}
    (w,) = decks.beam_species(m)
    assert w["name"] == "witness" and w["record"]["do_salame"] == 1 and w["source"] == "density_expr"
    assert w["args"]["expr"] == "n0" and w["args"]["constants"] == dict(n0=s["beam_density"])
    o = decks.salame_grid_current_moving_overload()
    assert o["beam_zmin"] == decks.salame_grid_current_overload()["beam_zmin"] == -3.0
    d = decks.salame_driver_witness()
    assert d["grid_current_on"] == 0 and d["beam_profile"] == 0 and d["beam_density"] == 0.5 and d["beam_charge"] == -1.0
    assert tuple(d["beam_pos_mean"]) == (0.0, 0.0, 3.0) and tuple(d["beam_pos_std"]) == (0.5, 0.5, 1.0)
    assert tuple(d["beam_umean"]) == (0.0, 0.0, 2000.0) and np.isfinite(d["beam_zmin"]) and np.isfinite(d["beam_zmax"])
    assert d["beam_zmin"] <= m["beam_zmin"] and d["beam_zmax"] > 3.0 + 2.5 and d["beam_zmax"] < d["hi"][2]
    assert d["dt"] != 0.0 and d["beam_do_salame"] == 0 and d["beam_species_salame"] == 1
    for k in ("nx", "ny", "nz", "lo", "hi", "order", "plasma_ppc", "mg_tol_rel", "beam_ppc"):
        assert d[k] == m[k], k
    (w,) = decks.beam_species(d)
    assert w["record"]["do_salame"] == 1 and w["args"]["constants"]["zw"] == m["beam_zmax"] and w["args"]["min_density"] > 0.0
    # the witness's density is its flat top inside the shared window and nothing outside
    from hipace_amd import expr
    prog = expr.compile_expr(w["args"]["expr"], ("x", "y", "z"), w["args"]["constants"])
    x = np.array([0.0, 0.29, 0.31, 0.0, 0.0]); y = np.zeros(5); z = np.array([0.0, 0.7, 0.0, 0.79, 3.0])
    assert np.array_equal(prog.evaluate(x, y, z), np.array([0.5, 0.5, 0.0, 0.0, 0.0]))


# ---- the pipeline's refusals ----------------------------------------------------------------------------------------------------
class _NoDevice:
    """stands where an engine would: any use beyond reading the deck fails the test"""

    def __init__(self, deck):
        self.deck = deck

    def __getattr__(self, name):
        raise AssertionError("the pipeline touched the engine (%s) before refusing the SALAME deck" % name)


@pytest.mark.parametrize("deck", [decks.salame_grid_current_moving(), decks.salame_driver_witness(),
                                  dict(R.vacuum_deck(), beam_species=[dict(particles=np.zeros((7, 1)), do_salame=1)])])
def test_pipeline_refuses_a_salame_species_without_touching_a_device(deck):
    e = _NoDevice(deck)
    for call in (lambda: pipeline.run_local_pipeline([e], 1, 0), lambda: pipeline.run_lanes([e], 0, 1, 1, 0),
                 lambda: next(pipeline._stage(e, 0, 1, 1, 0)), lambda: pipeline.run_pipeline(e, 0, 1, 1, 0)):
        with pytest.raises(NotImplementedError, match="beam_species_salame.*do_salame"):
            call()


# ---- the numpy restatements against themselves ---------------------------------------------------------------------------------
def test_numpy_deposit_conserves_the_current_and_is_linear_in_the_species():
    deck = R.vacuum_deck(order=2)
    species = S.three_species(base=1.0)
    soa = np.concatenate([s for _, s in species], axis=1)
    charges = np.concatenate([np.full(s.shape[1], r["charge"]) for r, s in species])
    inside = (np.abs(soa[0]) < 1.5) & (np.abs(soa[1]) < 1.5)           # the whole stencil inside the padded plane
    soa, charges = soa[:, inside], charges[inside]
    jx, jy, jz = M.deposit(deck, soa, charges)
    gam = np.sqrt(1.0 + (soa[3:6] ** 2).sum(axis=0))
    for plane, u in ((jx, soa[3]), (jy, soa[4]), (jz, soa[5])):
        terms = charges * soa[6] * u / gam
        assert abs(plane.sum() - terms.sum()) <= 1e-12 * np.abs(terms).sum()      # the shape factors add up to 1
    neg = charges < 0
    both = M.deposit(deck, soa, charges, live=neg) + M.deposit(deck, soa, charges, live=~neg)
    assert np.abs(both - np.array([jx, jy, jz])).max() <= 1e-13 * np.abs(jz).max()
    assert not M.deposit(deck, soa[:, :0], charges[:0]).any()
    for order in (0, 1, 2, 3):
        _, w = M.shape(order, np.linspace(-3.3, 7.7, 41))
        assert np.abs(sum(w) - 1.0).max() <= 4e-16


def test_numpy_scale_touches_the_selected_species_of_one_slice():
    bnd = np.array([0, 3, 3, 8]); nz = 3
    tags = np.array([0, 1, 1, 1, 0, 2, 1, 0], dtype=np.uint8)
    soa = np.zeros((7, 8)); soa[6] = np.arange(1.0, 9.0)
    w, sel = M.scale(soa, tags, bnd, nz, 0, [1], 1.75)                  # islice 0 = the last block
    assert sel.tolist() == [False, False, False, True, False, False, True, False]
    assert np.array_equal(w, np.array([1.0, 2.0, 3.0, 7.0, 5.0, 6.0, 12.25, 8.0]))
    w, sel = M.scale(soa, tags, bnd, nz, 1, [1], 1.75)                  # an empty slice
    assert not sel.any() and np.array_equal(w, soa[6])
    w, _ = M.scale(soa, tags, bnd, nz, 2, [1, 0], 0.0)
    assert np.array_equal(w, np.array([0.0, 0.0, 0.0, 4.0, 5.0, 6.0, 7.0, 8.0])) and not np.signbit(w).any()
    ez = np.arange(6.0).reshape(2, 3); jz = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 3.0]])
    assert M.weighted_mean_ez(ez, jz) == (1.0 + 15.0) / 4.0
