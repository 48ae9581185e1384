"""SALAME on a witness species of a moving-beam engine, on the GPU (salame/Salame.cpp, MultiBeam.cpp:42-59, 128-140).

Kernels alone, on the 32 x 32 x 12 vacuum box of tests/external_field_reference.py with beam_species_reference.three_species():
the species-masked deposit (k_beam_deposit_dyn<ORDER, 1, 1>) and SalameMultiplyBeamWeight on a slice of the container
(k_salame_scale_moving), through the two entry points the module itself calls.  The module, on the 64 x 64 x 100 SALAME box:
the moving engine against the static one (the code of the parent commit), slipping particles, a particle driver with a witness,
a bystander species, an overloaded witness, later steps, the adaptive step, the refusals, and "off means off".  Every
whole-deck run is made once per module and shared (_cached)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from hipace_amd import decks
from tests import beam_species_reference as S
from tests import external_field_reference as R
from tests import salame_moving_reference as M

pytestmark = pytest.mark.gpu

NZ = 12                                             # the vacuum box
# the tagged deposit's bound of tests/test_beam_species_gpu.py (ten times the run-to-run spread of the one-species deposit)
DEPOSIT_BOUND = 10 * 8.446e-16
# the project's bound for two runs of one deck (tests/test_salame_gpu.py: SI_W_MEASURED)
SI_W_MEASURED = 1.45e-13
W_BOUND = 10.0 * SI_W_MEASURED
WITNESS = list(range(47, 63))                       # slices of the witness in the SALAME decks (decks.py)
# Measured on the MI355X ("Moving beam"): moving against static -- W per slice 5.3e-15, per-particle weights 7.6e-15;
# slipping 6.1e-15; adaptive 5.6e-15; masked deposit against numpy 5.7e-16; driver + witness S1/|Ez_initial| = 6.4e-8 (S1 =
# 3.41e-9, S0 = 7.69e-2), fixed point 3.2e-6 (Bx), |W - 1| at iteration 0 of the reloaded species <= 1.8e-6.


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


# ------------------------------------------------------------------------------------------------------------------
# kernels alone
# ------------------------------------------------------------------------------------------------------------------
def _vacuum_deck(**kw):
    d = R.vacuum_deck(order=2)
    d.update(decks.SALAME_DEFAULT)
    d.update(beam_species_salame=1)
    d.update(kw)
    return d


def _vacuum_engine(api, step=None, insitu=False, begin=True, **kw):
    """species 0 = A (333), 1 = B (2600, do_salame: more than 2048 of them on slice 2), 2 = C (150)"""
    species = S.three_species(base=1.0)
    deck = S.one_species_deck(_vacuum_deck(**kw), species[0][0])
    eng = api.SliceEngine(deck, tile_size=0)
    assert eng.set_beam_particles(species[0][1]) == 0
    announced = dict(do_salame=1) if deck["beam_species_salame"] else {}
    assert eng.add_beam_species(name="B", particles=species[1][1], **announced, **species[1][0]) == 1
    assert eng.add_beam_species(name="C", particles=species[2][1], **species[2][0]) == 2
    if insitu:
        eng.set_insitu_beam()
    if step is not None:
        eng.set_step(step)
    if begin:
        eng.begin_step()
    return eng, species, deck


def _zero_slab(eng):
    from hipace_amd import _lib
    eng.sync()
    s = _lib.lib().hps_engine_slab(eng._h)
    z = np.zeros(s.ncomp * (s.ny + 2 * s.ng) * (s.nx + 2 * s.ng))
    _lib.check(_lib.lib().hps_memcpy_h2d(C.c_void_p(s.p), z.ctypes.data_as(C.c_void_p), z.nbytes))


def _held(tags, bnd, islice, k):
    a, b = M.slice_range(bnd, NZ, islice)
    return int((tags[a:b] == k).sum())


def test_masked_deposit_equals_numpy_for_every_subset_of_the_species(api):
    eng, species, deck = _vacuum_engine(api)
    bnd, soa, tags = eng.beam_container()
    charges = np.array([r["charge"] for r, _ in species])[tags]
    names = eng.comp_names()
    assert len(names) == 21 + 12
    targets = [names.index(n) for n in ("Salame_jx", "Salame_jy", "Salame_jz_beam")]
    # slice 2: A and more than 2048 of B; 3: A and B; 7: A and C; 0: A alone; 4 and 11: nobody
    slices = (2, 3, 7, 0, 4, 11)
    assert _held(tags, bnd, 2, 1) > 2048 and _held(tags, bnd, 3, 1) > 0 and _held(tags, bnd, 7, 2) > 0 and _held(tags, bnd, 7, 1) == 0
    assert _held(tags, bnd, 0, 0) > 0 and _held(tags, bnd, 0, 1) == 0 and _held(tags, bnd, 0, 2) == 0
    assert bnd[NZ - 4] == bnd[NZ - 1 - 4] and bnd[1] == bnd[0]
    worst = 0.0
    for r in (1, 2, 3):
        for subset in itertools.combinations((0, 1, 2), r):
            for k in slices:
                _zero_slab(eng)
                eng.deposit_beam_species(k, subset, jx="Salame_jx", jy="Salame_jy", jz="Salame_jz_beam")
                slab = eng.slab()
                a, b = M.slice_range(bnd, NZ, k)
                live = np.isin(tags[a:b], subset)
                untouched = [c for c in range(len(names)) if c not in targets]
                assert not slab[untouched].any(), (subset, k)
                if not live.any():          # an empty slice, or one that holds unselected species only: exactly zero
                    assert not slab.any(), (subset, k)
                    continue
                ref = M.deposit(deck, soa[:, a:b], charges[a:b], live=live)
                for q, c in enumerate(targets):
                    scale = np.abs(ref[q]).max()
                    err = np.abs(slab[c] - ref[q]).max() / scale
                    worst = max(worst, err)
                    assert err <= DEPOSIT_BOUND, (subset, k, names[c], err)
    print(f"masked deposit: worst plane-wise difference from numpy {worst:.3e} of the plane's maximum (bound {DEPOSIT_BOUND:.1e})")
    # jz alone leaves the jx, jy planes; the instance is on record under its three-index name, the tagged deposit's is not
    _zero_slab(eng)
    eng.deposit_beam_species(2, (1,), jz="Salame_jz_beam")
    slab = eng.slab()
    assert slab[targets[2]].any() and not slab[[c for c in range(len(names)) if c != targets[2]]].any()
    assert eng.beam_kernels() == ({"k_beam_deposit_dyn<2,1,1>"}, True)


@pytest.mark.parametrize("islice", [2, 3])
def test_scale_multiplies_the_selected_species_of_one_slice_bit_for_bit(api, islice):
    eng, _, _ = _vacuum_engine(api)
    bnd, soa, tags = eng.beam_container()
    a, b = M.slice_range(bnd, NZ, islice)
    nB = _held(tags, bnd, islice, 1)
    if islice == 2:
        assert nB > 2048                                  # the slice above 2048
    else:
        assert nB > 0 and nB % 64 != 0 and (b - a) % 64 != 0
    assert _held(tags, bnd, islice, 0) > 0                # another species shares the slice
    W = 1.75                                              # w * W is one rounding
    eng.salame_scale_slice(islice, W)
    bnd1, soa1, tags1 = eng.beam_container()
    ref_w, sel = M.scale(soa, tags, bnd, NZ, islice, [1], W)
    assert sel.sum() == nB
    assert np.array_equal(soa1[6], ref_w)                 # the selected weights exactly w * W, every other weight as it was
    assert np.array_equal(soa1[:6], soa[:6]) and np.array_equal(bnd1, bnd) and np.array_equal(tags1, tags)
    # a slice without the species (0: A alone; 7: A and C) and an empty one (4): nothing changes
    for k in (0, 7, 4):
        eng.salame_scale_slice(k, W)
    assert np.array_equal(eng.beam_container()[1], soa1)
    assert eng.beam_kernels()[0] == set()                 # (no deposit, no push: the scaling is not a beam kernel instance)


def test_scale_by_zero_removes_the_particles(api):
    """W = 0: weight exactly 0, out of the per-species in-situ count, not moved by the next push (the state the push's
    absorbing boundary leaves a particle in).  The step is begun as step 1, so that no SALAME module runs."""
    eng, _, _ = _vacuum_engine(api, step=1, insitu=True)
    bnd, soa, tags = eng.beam_container()
    eng.salame_scale_slice(2, 0.0)
    _, soa1, _ = eng.beam_container()
    ref_w, sel = M.scale(soa, tags, bnd, NZ, 2, [1], 0.0)
    assert sel.sum() > 2048 and np.array_equal(soa1[6], ref_w) and not np.signbit(soa1[6][sel]).any()
    for k in range(NZ - 1, -1, -1):
        eng.solve_slice(k)
    _, soa2, tags2 = eng.beam_container()
    gone = (tags2 == 1) & (soa2[6] == 0.0)
    assert gone.sum() == sel.sum()
    key = lambda s: s[:6][:, np.lexsort(s[:6])]
    assert np.array_equal(key(soa2[:, gone]), key(soa1[:, sel]))                  # where they were, with the momenta they had
    live = (tags2 == 1) & (soa2[6] != 0.0)
    assert live.sum() == (tags == 1).sum() - sel.sum()
    was = (tags == 1) & ~sel
    assert not np.array_equal(key(soa2[:, live])[0], key(soa[:, was])[0])         # ... while the others of the species moved
    ins = eng.insitu_beam(species=1)
    assert ins["Np"][2] == 0.0 and ins["sum(w)"][2] == 0.0
    assert ins["Np"][3] == float(_held(tags, bnd, 3, 1)) and ins["Np"].sum() == float(live.sum())
    assert eng.insitu_beam(species=0)["Np"][2] == float(_held(tags, bnd, 2, 0))
    # begun as step 1: no species-masked instance was launched
    assert not any(n.endswith(",1,1>") for n in eng.beam_kernels()[0])


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
def _static_run(api, deck, insitu=False):
    """the static-beam SALAME engine (the code of the parent commit): the reference of the moving runs"""
    eng = api.SliceEngine(deck)
    bnd, beam0 = eng.beam_state()                      # the deck's own beam as generated
    beam0 = beam0.copy()
    eng.set_diagnostics(True)
    if insitu:
        eng.set_insitu_beam()
    eng.run_step()
    r = dict(deck=deck, beam0=beam0, stats=eng.salame_stats(), checksums=eng.checksums())
    r["bnd"], r["beam"] = eng.beam_state()
    if insitu:
        r["insitu"] = eng.insitu_beam()
    return r


def _moving_engine(api, deck, driver=None, witness=None, extra=(), fields=None, insitu=False, salame=True):
    """driver / witness: host particles in place of the deck's generators; extra: further species (add_beam_species keywords)"""
    d = dict(deck)
    own = d.pop("beam_species")
    if not salame:
        d["beam_species_salame"] = 0
    if driver is not None:
        d["beam_profile"] = -1
    eng = api.SliceEngine(d)
    if driver is not None:
        eng.set_beam_particles(driver, allow_outside=True)
    w = dict(own[0]) if witness is None else dict(name="witness", do_salame=1, particles=witness)
    if not salame:
        w.pop("do_salame")
    assert eng.add_beam_species(**w) == 1
    for k, spec in enumerate(extra, 2):
        assert eng.add_beam_species(**spec) == k
    eng.set_diagnostics(True)
    if fields:
        eng.set_field_diagnostic(list(fields))
    if insitu:
        eng.set_insitu_beam()
    return eng


def _record(eng, r, key, fields=None, insitu=False, salame=True):
    r[key] = dict(container=eng.beam_container(), checksums=eng.checksums(), kernels=eng.beam_kernels()[0])
    if salame:
        r[key]["stats"] = eng.salame_stats()
    if fields:
        r[key]["fd"] = eng.field_diagnostic()
    if insitu:
        r[key]["insitu"] = eng.insitu_beam(species=1)


def _moving_run(api, deck, steps=1, adaptive_dt=None, keep_slab=False, fields=None, insitu=False, salame=True, **kw):
    eng = _moving_engine(api, deck, fields=fields, insitu=insitu, salame=salame, **kw)
    r = dict(deck=deck, container0=eng.beam_container())
    for step in range(steps):
        if adaptive_dt is not None:
            eng.set_time(step * adaptive_dt, adaptive_dt)
        eng.run_step()
        _record(eng, r, f"step{step}", fields=fields, insitu=insitu, salame=salame)
        if keep_slab and step == 0:
            r["slab"], r["names"] = eng.slab(), eng.comp_names()
    return r


_CACHE = {}
SLIP = dict(beam_umean=(0.0, 0.0, 20.0), beam_ppc=(4, 4, 2))      # case 4: a slow witness in two z layers per slice
SLIP_DT = 50.0


def _species(r, key, k):
    """species k's particles of a recorded container, in container order -> (7, n)"""
    bnd, soa, tags = r[key]["container"] if key != "container0" else r["container0"]
    return soa[:, tags == k]


def _driver_and_witness(api, which):
    """the two species of the driver + witness run as host particles: as generated, or as step 0 left them"""
    a = _cached(api, "dw")
    key = "container0" if which == "initial" else "step0"
    return _species(a, key, 0), _species(a, key, 1)


def _bystander(witness0):
    """case 6: a weak electron species on the witness's slices -- a tenth of its density (0.05), its radius, u_x = 0.5, a little
    off its lattice"""
    b = np.array(witness0)
    b[0] += 0.03; b[1] -= 0.02
    b[3] = 0.5
    b[6] *= 0.1
    return b


def _cached(api, name):
    if name in _CACHE:
        return _CACHE[name]
    if name == "static":
        r = _static_run(api, decks.salame_grid_current())
    elif name == "moving":                  # the static deck's own beam as species 1 of the moving twin; two steps
        r = _moving_run(api, decks.salame_grid_current_moving(), witness=_cached(api, "static")["beam0"], steps=2)
    elif name == "moving_generated":        # ... and the deck as it stands: the witness from the device's fixed_ppc generator
        r = _moving_run(api, decks.salame_grid_current_moving())
    elif name == "adaptive":
        d = decks.salame_grid_current_moving()
        d.update(decks.ADAPTIVE_DEFAULT)
        d.update(dt_adaptive=1, nt_per_betatron=20.0)
        r = _moving_run(api, d, witness=_cached(api, "static")["beam0"], adaptive_dt=d["dt"])
    elif name == "slip_static":
        d = decks.salame_grid_current(); d.update(SLIP)
        r = _static_run(api, d)
    elif name == "slip_moving":
        d = decks.salame_grid_current_moving(dt=SLIP_DT); d.update(SLIP)
        r = _moving_run(api, d, witness=_cached(api, "slip_static")["beam0"])
    elif name == "overload_static":
        r = _static_run(api, decks.salame_grid_current_overload(), insitu=True)
    elif name == "overload_moving":
        r = _moving_run(api, decks.salame_grid_current_moving_overload(), witness=_cached(api, "overload_static")["beam0"],
                        steps=2, insitu=True)
    elif name == "dw":
        r = _moving_run(api, decks.salame_driver_witness(), fields=("Ez",))
    elif name == "dw_plain":                # the same two species without SALAME
        r = _moving_run(api, decks.salame_driver_witness(), fields=("Ez",), salame=False)
    elif name == "dw_reloaded_plain":       # both final species in a fresh two-species engine without SALAME
        dr, wi = _driver_and_witness(api, "final")
        r = _moving_run(api, decks.salame_driver_witness(), driver=dr, witness=wi, salame=False)
    elif name == "dw_reloaded_salame":      # ... and with SALAME: a fixed point
        dr, wi = _driver_and_witness(api, "final")
        r = _moving_run(api, decks.salame_driver_witness(), driver=dr, witness=wi)
    elif name == "dw_reloaded_salame_1":    # one iteration only: its W is the W of iteration 0
        dr, wi = _driver_and_witness(api, "final")
        d = decks.salame_driver_witness(); d["salame_n_iter"] = 1
        r = _moving_run(api, d, driver=dr, witness=wi)
    elif name == "bystander":               # case 6: the witness with a small u_x and a bystander species, two steps
        dr, wi = _driver_and_witness(api, "initial")
        wi = np.array(wi); wi[3] = 0.01
        r = _moving_run(api, decks.salame_driver_witness(), driver=dr, witness=wi, steps=2, keep_slab=True, fields=("jx_beam",),
                        extra=[dict(name="bystander", particles=_bystander(wi))])
    _CACHE[name] = r
    return r


def _slice_of(deck, z):
    dz = (deck["hi"][2] - deck["lo"][2]) / deck["nz"]
    return np.floor((z - deck["lo"][2]) / dz).astype(int)


def _sorted_weights_per_slice(bnd, w, nz, slices):
    return {k: np.sort(w[slice(*M.slice_range(bnd, nz, k))]) for k in slices}


def _witness_weights_per_slice(r, key, slices):
    bnd, soa, tags = r[key]["container"]
    nz = r["deck"]["nz"]
    out = {}
    for k in slices:
        a, b = M.slice_range(bnd, nz, k)
        out[k] = np.sort(soa[6, a:b][tags[a:b] == 1])
    return out


def _compare_stats(m, s, slices, what):
    assert np.array_equal(m["iterations"], s["iterations"]), what
    assert np.array_equal(m["converged"], s["converged"]) and np.array_equal(m["overloaded"], s["overloaded"]), what
    assert np.array_equal(m["ran"], s["ran"]) and np.flatnonzero(s["ran"]).tolist() == list(slices)
    live = s["W"] != 0.0
    assert np.array_equal(m["W"] != 0.0, live)
    relW = np.abs(m["W"][live] / s["W"][live] - 1.0).max()
    print(f"{what}: W per slice differs by {relW:.3e} (bound {W_BOUND:.2e}); iterations {s['iterations'][list(slices)]}")
    assert relW <= W_BOUND, what
    return relW


# ---- 3. moving equals static --------------------------------------------------------------------------------------------------
def test_moving_engine_scales_the_weights_the_static_engine_does(api):
    """salame_grid_current_moving with the static deck's own beam as species 1 against salame_grid_current on the static engine:
    the same wake, the same module, the container and the tagged kernels in place of the slice blocks."""
    s, m = _cached(api, "static"), _cached(api, "moving")
    _compare_stats(m["step0"]["stats"], s["stats"], WITNESS, "moving against static")
    nz = s["deck"]["nz"]
    ws = _sorted_weights_per_slice(s["bnd"], s["beam"][6], nz, WITNESS)
    wm = _witness_weights_per_slice(m, "step0", WITNESS)
    worst = 0.0
    for k in WITNESS:
        assert ws[k].size == wm[k].size > 0
        worst = max(worst, np.abs(wm[k] / ws[k] - 1.0).max())
    print(f"moving against static: per-particle weights differ by {worst:.3e} (bound {W_BOUND:.2e})")
    assert worst <= W_BOUND
    bnd, soa, tags = m["step0"]["container"]
    assert (tags == 1).all() and soa.shape[1] == s["beam"].shape[1]          # species 0 is empty behind the grid current
    assert "k_beam_deposit_dyn<2,1,1>" in m["step0"]["kernels"]


def test_the_moving_deck_as_it_stands_loads_its_generated_witness(api):
    """The deck's own witness (the device's fixed_ppc generator on the flat top written as a density) instead of host particles:
    the same slices run, converge and are not overloaded.  The two generators build the same physical beam; the weight factors'
    difference from the static run's is printed, and held to the 5 % sanity band of the other variants of the deck."""
    s, g = _cached(api, "static"), _cached(api, "moving_generated")
    st = g["step0"]["stats"]
    assert np.flatnonzero(st["ran"]).tolist() == WITNESS and not st["overloaded"].any() and (st["W"][WITNESS] > 0.0).all()
    assert ((st["converged"] | (st["iterations"] == 5))[WITNESS]).all()
    rel = np.abs(st["W"][WITNESS] / s["stats"]["W"][WITNESS] - 1.0).max()
    print(f"generated witness: W per slice differs from the static run's by {rel:.3e}")
    assert rel < 0.05


# ---- 4. slipping --------------------------------------------------------------------------------------------------------------
def test_a_particle_is_scaled_on_its_original_slice_once(api):
    """A slow witness (u_z = 20) in two z layers per slice and a step long enough for the lower layer to slip into the next
    slice during step 0: it arrives scaled, is pushed there and must not be scaled again (nor have missed its own slice's
    scaling).  A double or missed scaling is off by a factor of 0.8 - 4 (the W of neighbouring slices)."""
    s, m = _cached(api, "slip_static"), _cached(api, "slip_moving")
    nz = s["deck"]["nz"]
    bnd0 = m["container0"][0]
    bnd1, soa1, tags1 = m["step0"]["container"]
    count0 = {k: M.slice_range(bnd0, nz, k)[1] - M.slice_range(bnd0, nz, k)[0] for k in range(nz)}
    count1 = {k: M.slice_range(bnd1, nz, k)[1] - M.slice_range(bnd1, nz, k)[0] for k in range(nz)}
    out = {nz: 0}
    for k in range(nz - 1, 0, -1):        # what slice k handed to slice k - 1 (nobody slips through two slices of this deck)
        out[k] = count0[k] + out[k + 1] - count1[k]
    partial = [k for k in WITNESS if 0 < out[k] < count0[k]]
    print("slipping: handed on per witness slice", [out[k] for k in WITNESS], "of", [count0[k] for k in WITNESS])
    assert all(out[k] >= 0 for k in out) and len(partial) >= 8
    ms, ss = m["step0"]["stats"], s["stats"]
    print("slipping: iterations", ms["iterations"][WITNESS], "static", ss["iterations"][WITNESS],
          "W differs by", np.abs(ms["W"][WITNESS] / ss["W"][WITNESS] - 1.0).max())
    assert np.flatnonzero(ms["ran"]).tolist() == WITNESS and not ms["overloaded"].any()
    ws, wm = np.sort(s["beam"][6]), np.sort(soa1[6][tags1 == 1])
    assert ws.size == wm.size
    rel = np.abs(wm / ws - 1.0).max()
    print(f"slipping: sorted weights differ from the static run's by {rel:.3e} (bound {W_BOUND:.2e})")
    assert rel <= W_BOUND


# ---- 5. driver and witness ----------------------------------------------------------------------------------------------------
def _witness_jz(r, key):
    """the witness's own jz on its slices: the numpy deposit of its particles as the step left them (u = (0, 0, 2000): the push
    moves them by less than 1e-6 of a cell)"""
    deck = r["deck"]
    _, _, _, _, _, g, _ = M.geometry(deck)
    bnd, soa, tags = r[key]["container"]
    out = {}
    for k in WITNESS:
        a, b = M.slice_range(bnd, deck["nz"], k)
        live = tags[a:b] == 1
        out[k] = M.deposit(deck, soa[:, a:b], np.full(b - a, deck["beam_charge"]), live=live)[2][g:-g, g:-g]
    return out


BEAM_TRANSVERSE = ("N_jx_beam", "N_jy_beam", "jx_beam", "jy_beam", "P_jx_beam", "P_jy_beam")


def _worst_checksum_difference(a, c):
    """largest relative difference of the checksums c from a.  The transverse beam currents are an exact 0 in step 0 of the run
    that generated its beams (u_x = u_y = 0 until the push, which follows the deposits); the reloaded species carry what that
    push gave them: those planes are held to the same fraction of the jz_beam checksum instead."""
    worst, worst_k = 0.0, None
    for k, v in a.items():
        if v == 0.0 and c[k] == 0.0:
            continue
        if v == 0.0:
            assert k in BEAM_TRANSVERSE, k
            rel = abs(c[k]) / abs(a["jz_beam"])
        else:
            rel = abs(c[k] - v) / abs(v)
        if rel > worst:
            worst, worst_k = rel, k
    return worst, worst_k


def test_salame_flattens_ez_behind_a_particle_driver(api):
    a, b = _cached(api, "dw"), _cached(api, "dw_plain")
    deck = a["deck"]
    dz = (deck["hi"][2] - deck["lo"][2]) / deck["nz"]
    S1, ez0 = M.flatness(a["step0"]["fd"]["Ez"], _witness_jz(a, "step0"), WITNESS, dz, deck["lo"][2])
    S0, ez0b = M.flatness(b["step0"]["fd"]["Ez"], _witness_jz(b, "step0"), WITNESS, dz, deck["lo"][2])
    st = a["step0"]["stats"]
    print(f"driver + witness: Ez_initial {ez0:.6f} (plain {ez0b:.6f}) S1 {S1:.3e} S0 {S0:.3e} S1/|Ez_initial| {S1 / abs(ez0):.3e}")
    print("W", st["W"][WITNESS], "iterations", st["iterations"][WITNESS], "converged", st["converged"][WITNESS])
    assert ez0 < 0.0
    assert np.flatnonzero(st["ran"]).tolist() == WITNESS and not st["overloaded"].any() and (st["W"][WITNESS] > 0.0).all()
    assert ((st["converged"] | (st["iterations"] == 5))[WITNESS]).all()
    assert S1 <= S0 / 20.0
    # the driver's weights are bit-unchanged, the witness's are not
    d0, d1 = _species(a, "container0", 0), _species(a, "step0", 0)
    assert d0.shape[1] > 0 and np.array_equal(d1[6], d0[6])
    w0, w1 = _species(a, "container0", 1), _species(a, "step0", 1)
    assert w0.shape == w1.shape and (w1[6] != w0[6]).all()
    assert {"k_beam_deposit_dyn<2,1,1>", "k_beam_deposit_dyn<2,1>", "k_beam_push<2,0,1>"} <= a["step0"]["kernels"]


def test_driver_and_witness_is_a_fixed_point_and_step_4_is_consistent(api):
    a, c = _cached(api, "dw"), _cached(api, "dw_reloaded_plain")
    worst, worst_k = _worst_checksum_difference(a["step0"]["checksums"], c["step0"]["checksums"])
    print(f"driver + witness fixed point: largest relative checksum difference {worst:.3e} ({worst_k})")
    assert worst < 1e-5, "step 4 is inconsistent with a plain solve of the scaled witness behind the driver"
    tol = 1.0e-4          # salame_relative_tolerance's default
    s2, s1 = _cached(api, "dw_reloaded_salame")["step0"]["stats"], _cached(api, "dw_reloaded_salame_1")["step0"]["stats"]
    print("reloaded: iterations", s2["iterations"][WITNESS], "|W - 1| at iteration 0", np.abs(s1["W"][WITNESS] - 1.0))
    assert (s2["iterations"][WITNESS] == 2).all() and s2["converged"][WITNESS].all()
    assert (s1["iterations"][WITNESS] == 1).all()
    assert (np.abs(s1["W"][WITNESS] - 1.0) < 100.0 * tol).all()


# ---- 6. the mask inside the module --------------------------------------------------------------------------------------------
def _rounding_bound(contributions):
    """two sums (the device's, numpy's) of `contributions` terms each, every addition rounded against at most the sum of the
    terms' magnitudes: 2 n 2^-53 of that sum"""
    return 2.0 * contributions * 2.0 ** -53


def test_the_module_deposits_the_salame_species_alone_and_step_0_leaves_its_jx_out(api):
    """Driver, witness (u_x = 0.01) and a bystander electron species (u_x = 0.5) on the witness's slices.  16 particles per
    cell and species, 9 cells each: at most 144 terms per cell and species."""
    r = _cached(api, "bystander")
    deck = r["deck"]
    nz = deck["nz"]
    _, _, _, _, _, g, _ = M.geometry(deck)
    bnd0, soa0, tags0 = r["container0"]
    bnd1, soa1, tags1 = r["step0"]["container"]
    assert np.array_equal(bnd0, bnd1) and np.array_equal(tags0, tags1)          # nobody slips: the container keeps its order
    st = r["step0"]["stats"]
    assert np.flatnonzero(st["ran"]).tolist() == WITNESS and not st["overloaded"].any()
    # (a) the SALAME slice's jz_beam after the step: the last witness slice's last STEP 3, the witness alone at the weights
    #     before the last scaling, where it stood before the push
    last = WITNESS[0]
    a, b = M.slice_range(bnd0, nz, last)
    before = np.array(soa0[:, a:b])
    before[6] = np.where(tags0[a:b] == 1, soa1[6, a:b] / st["W"][last], soa0[6, a:b])
    charges = np.full(b - a, deck["beam_charge"])
    assert (tags0[a:b] == 0).any() and (tags0[a:b] == 1).any() and (tags0[a:b] == 2).any()
    ref = M.deposit(deck, before, charges, live=tags0[a:b] == 1)[2]
    got = r["slab"][r["names"].index("Salame_jz_beam")]
    err = np.abs(got - ref).max() / np.abs(ref).max()
    everyone = M.deposit(deck, before, charges)[2]
    print(f"Salame_jz_beam against the witness alone: {err:.3e} (every species: {np.abs(got - everyone).max() / np.abs(ref).max():.3e})")
    assert err <= _rounding_bound(144)
    assert np.abs(got - everyone).max() / np.abs(ref).max() > 1e-3               # ... and not the three of them
    # (b) step 0's jx_beam: the bystander's and the driver's currents (the driver's u_x is an exact 0 when it deposits), not
    #     the witness's (a fifth of the bystander's)
    jx0, jx1 = r["step0"]["fd"]["jx_beam"], r["step1"]["fd"]["jx_beam"]
    worst0 = worst1 = seen = 0.0
    for k in WITNESS:
        a, b = M.slice_range(bnd0, nz, k)
        charges = np.full(b - a, deck["beam_charge"])
        ref0 = M.deposit(deck, soa0[:, a:b], charges, live=tags0[a:b] != 1)[0][g:-g, g:-g]
        wit0 = M.deposit(deck, soa0[:, a:b], charges, live=tags0[a:b] == 1)[0][g:-g, g:-g]
        scale = np.abs(ref0).max()
        worst0 = max(worst0, np.abs(jx0[k] - ref0).max() / scale)
        seen = max(seen, np.abs(wit0).max() / scale)
        # (c) step 1's: all three, from the container as step 0 left it
        ref1 = M.deposit(deck, soa1[:, a:b], charges)[0][g:-g, g:-g]
        mag1 = M.deposit(deck, soa1[:, a:b], charges, absolute=True)[0][g:-g, g:-g]
        worst1 = max(worst1, np.abs(jx1[k] - ref1).max() / mag1.max())
        assert np.abs(jx1[k] - jx0[k]).max() > 0.05 * scale                      # (the witness's share is in it now)
    print(f"jx_beam: step 0 against bystander + driver {worst0:.3e} (the witness would add {seen:.3e}); step 1 against all {worst1:.3e}")
    assert seen > 0.05
    assert worst0 <= _rounding_bound(2 * 144)
    assert worst1 <= _rounding_bound(3 * 144)


# ---- 7. overload --------------------------------------------------------------------------------------------------------------
def test_overload_drops_the_rest_of_the_witness_for_good(api):
    s, m = _cached(api, "overload_static"), _cached(api, "overload_moving")
    wit = list(range(36, 63))
    st = m["step0"]["stats"]
    assert np.array_equal(st["overloaded"], s["stats"]["overloaded"]) and np.flatnonzero(st["ran"]).tolist() == wit
    over = np.flatnonzero(st["overloaded"])
    assert len(over) > 0 and over.tolist() == list(range(36, over.max() + 1)) and over.max() < 62
    nz = s["deck"]["nz"]
    bnd, soa, tags = m["step0"]["container"]
    w0 = _witness_weights_per_slice(m, "step0", wit)
    for k in wit:
        if k in over:
            assert w0[k].size > 0 and not w0[k].any() and not np.signbit(w0[k]).any()        # exactly 0
        else:
            assert (w0[k] > 0.0).all()
    ins = m["step0"]["insitu"]
    held = np.array([w0[k].size for k in wit], dtype=float)
    kept = np.array([k not in over for k in wit])
    assert (ins["Np"][over] == 0.0).all() and (ins["sum(w)"][over] == 0.0).all()             # out of the in-situ count
    assert np.array_equal(ins["Np"][wit][kept], held[kept])
    # after step 1 they are still gone, and the remaining weights are what step 0 left
    _, soa1, tags1 = m["step1"]["container"]
    assert np.array_equal(np.sort(soa1[6][tags1 == 1]), np.sort(soa[6][tags == 1]))
    assert (m["step1"]["insitu"]["Np"][over] == 0.0).all()
    assert m["step1"]["insitu"]["Np"].sum() == held[kept].sum()
    assert all(np.isfinite(v) for v in m["step1"]["checksums"].values())


# ---- 8. later steps and the adaptive step -------------------------------------------------------------------------------------
def test_later_steps_keep_the_weights_and_launch_no_masked_deposit(api):
    m = _cached(api, "moving")
    assert "k_beam_deposit_dyn<2,1,1>" in m["step0"]["kernels"]
    assert m["step1"]["kernels"] - m["step0"]["kernels"] <= {"k_beam_deposit_dyn<2,1>"}      # (step 0's Next deposit had no taker)
    _, soa0, tags0 = m["step0"]["container"]
    _, soa1, tags1 = m["step1"]["container"]
    assert np.array_equal(np.sort(soa1[6][tags1 == 1]), np.sort(soa0[6][tags0 == 1]))
    for key in ("W", "W_total", "iterations", "converged", "overloaded"):
        assert np.array_equal(m["step1"]["stats"][key], m["step0"]["stats"][key]), key
    # an engine that begins at step 1 never launches the masked instance: its deposits are the tagged ones
    eng, _, _ = _vacuum_engine(api, step=1)
    for k in range(NZ - 1, -1, -1):
        eng.solve_slice(k)
    assert eng.beam_kernels() == ({"k_beam_push<2,0,1>", "k_beam_deposit_dyn<2,1>", "k_beam_partition<0,1>"}, True)
    assert not eng.salame_stats()["ran"].any()


def test_adaptive_step_loads_the_same_weights(api):
    """hipace.dt = adaptive: SALAME precedes every push, the moments are reduced behind it"""
    f, a = _cached(api, "moving"), _cached(api, "adaptive")
    _compare_stats(a["step0"]["stats"], f["step0"]["stats"], WITNESS, "adaptive against fixed dt")
    wf, wa = _witness_weights_per_slice(f, "step0", WITNESS), _witness_weights_per_slice(a, "step0", WITNESS)
    worst = max(np.abs(wa[k] / wf[k] - 1.0).max() for k in WITNESS)
    print(f"adaptive against fixed dt: per-particle weights differ by {worst:.3e} (bound {W_BOUND:.2e})")
    assert worst <= W_BOUND
    assert "k_beam_partition<1,1>" in a["step0"]["kernels"]


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_leave_the_engine_usable(api):
    from hipace_amd import _lib, pipeline
    base = decks.salame_grid_current_moving
    d = base(); d["dt"] = 0.0
    with pytest.raises(_lib.HpsError, match="beam_species_salame needs a moving beam .* a static beam \\(dt = 0\\) has no species"):
        api.SliceEngine(d)
    d = base(); d["bxby_solver"] = 1
    with pytest.raises(_lib.HpsError, match="beam_species_salame needs the explicit solver .* predictor-corrector"):
        api.SliceEngine(d)
    d = decks.with_ion_species(base(), "H", 1.0); d["background_density_SI"] = 1.0e23
    with pytest.raises(_lib.HpsError, match="beam_species_salame with the ionisable species"):
        api.SliceEngine(d)
    d = base(); d.update(laser_on=1, laser_a0=1.0)
    with pytest.raises(_lib.HpsError, match="beam_species_salame with a laser"):
        api.SliceEngine(d)
    d = decks.salame_grid_current(); d["beam_species_salame"] = 1
    with pytest.raises(_lib.HpsError, match="the deck has beam_do_salame"):
        api.SliceEngine(d)

    soa = S.three_species()[2][1]
    # do_salame without the deck's announcement; the engine goes on as a two-species engine without SALAME
    eng, _, _ = _vacuum_engine(api, begin=False, beam_species_salame=0)
    with pytest.raises(_lib.HpsError, match="a do_salame species needs beam_species_salame"):
        eng.add_beam_species(particles=soa, do_salame=1)
    assert eng.beam_species() == (["beam", "B", "C"], [333, 2600, 150])
    with pytest.raises(_lib.HpsError, match="beam_do_salame"):
        eng.salame_stats()
    eng.run_step()
    assert eng.beam_kernels() == ({"k_beam_push<2,0,1>", "k_beam_deposit_dyn<2,1>", "k_beam_partition<0,1>"}, True)

    # a gaussian fixed_weight source without zmin / zmax for such a species; it stays empty and can be filled afterwards
    eng = api.SliceEngine(_vacuum_deck(background_density_SI=1.0e23, plasma_ppc=(1, 1), plasma_density=1.0), tile_size=0)
    eng.set_beam_particles(S.three_species()[0][1])
    gauss = dict(num_particles=1000, position_mean=(0.0, 0.0, 0.0), position_std=(0.3, 0.3, 0.5), u_mean=(0.0, 0.0, 30.0), density=1.0)
    with pytest.raises(_lib.HpsError, match="a do_salame beam species needs the can profile, or zmin and zmax"):
        eng.add_beam_species(do_salame=1, fixed_weight=gauss)
    assert eng.beam_species() == (["beam", "beam1"], [333, 0])
    eng.set_beam_fixed_weight(species=1, **dict(gauss, zmin=-1.0, zmax=1.0))
    assert eng.beam_species()[1][1] > 0
    # a beam collision with several species stays refused
    with pytest.raises(_lib.HpsError, match="the engine holds several beam species"):
        eng.add_beam_collision(0, 5.0, 1)
    eng.run_step()
    assert eng.salame_stats()["ran"].any()
    # the entry points on a static-beam engine, and before the first step
    static = api.SliceEngine(dict(_vacuum_deck(beam_species_salame=0), dt=0.0), tile_size=0)
    with pytest.raises(_lib.HpsError, match="hps_engine_deposit_beam_species: needs a moving beam"):
        static.deposit_beam_species(2, (0,), jz="jz_beam")
    with pytest.raises(_lib.HpsError, match="hps_engine_salame_scale_slice: needs a moving beam"):
        static.salame_scale_slice(2, 1.5)
    eng, _, _ = _vacuum_engine(api, begin=False)
    with pytest.raises(_lib.HpsError, match="call after hps_engine_begin_step"):
        eng.salame_scale_slice(2, 1.5)
    with pytest.raises(_lib.HpsError, match="call after hps_engine_begin_step"):
        eng.deposit_beam_species(2, (0,), jz="jz_beam")
    eng.begin_step()
    with pytest.raises(_lib.HpsError, match="no such slice"):
        eng.salame_scale_slice(NZ, 1.5)
    with pytest.raises(_lib.HpsError, match="cjx and cjy go together"):
        eng.deposit_beam_species(2, (0,), jx="jx_beam")
    # the three pipeline entry points
    eng = api.SliceEngine(_vacuum_deck(), tile_size=0)
    for call in (lambda: pipeline.run_local_pipeline([eng], 1, 0), lambda: pipeline.run_lanes([eng], 0, 1, 1, 0),
                 lambda: pipeline.run_pipeline(eng, 0, 1, 1, 0)):
        with pytest.raises(NotImplementedError, match="beam_species_salame"):
            call()


# ---- 10. off means off --------------------------------------------------------------------------------------------------------
PARENT_INFO = (21, 2, 0)        # hps_engine_info of the vacuum box at the parent commit: components, guard cells, plasma particles
PARENT_KERNELS = {"k_beam_push<2,0,1>", "k_beam_deposit_dyn<2,1>", "k_beam_partition<0,1>"}


@pytest.mark.parametrize("extra", [{}, dict(decks.SALAME_DEFAULT, **decks.SALAME_SPECIES_DEFAULT),
                                   dict(beam_do_salame=0, beam_species_salame=0, salame_n_iter=3, salame_relative_tolerance=1e-2,
                                        salame_no_advance=1, salame_Ez_target_slope=0.5)])
def test_off_means_off(api, extra):
    """A three-species moving engine without SALAME launches the kernel instances and allocates the components it did at the
    parent commit, whether the new keys are absent, zero, or -- all but the switches -- set."""
    from hipace_amd import _lib
    species = S.three_species()
    deck = S.one_species_deck(dict(R.vacuum_deck(order=2), **extra), species[0][0])
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_beam_particles(species[0][1])
    for k in (1, 2):
        eng.add_beam_species(particles=species[k][1], **species[k][0])
    assert (eng.ncomp, eng.ng, eng.nparticles) == PARENT_INFO
    assert _lib.lib().hps_engine_slab(eng._h).ncomp == PARENT_INFO[0]
    assert len(eng.comp_names()) == PARENT_INFO[0]
    eng.run_step()
    eng.run_step()
    assert eng.beam_kernels() == (PARENT_KERNELS, True)
    with pytest.raises(_lib.HpsError, match="beam_do_salame"):
        eng.salame_stats()
    # ... and the engine that did announce a SALAME species keeps hps_engine_info without the twelve planes
    sal, _, _ = _vacuum_engine(api, begin=False)
    assert (sal.ncomp, sal.ng, sal.nparticles) == PARENT_INFO and _lib.lib().hps_engine_slab(sal._h).ncomp == PARENT_INFO[0] + 12
