"""Which tiled particle kernel instances the ENGINE launches, deck by deck.

tests/test_particle_dispatch_gpu.py pins every instance the four tiled launchers can pick, through the C entries.  The engine
reaches the same launchers through its own schedule (Engine::species_deposit / species_explicit / species_advance,
push_with_ionization, the gated push, the fused push + deposition, the neutralising background), which decides per species
and per slice what each launch is given: the laser's |a|^2, the valid-by-weight and valid-by-psi_half variants, the ions' ADK
arguments, the tile size.  Each case below runs one short deck with the dispatch record on (hps_particles_record) and holds
the set of recorded instances to a literal set.

The literal sets were written from a run of the library of the commit BEFORE the launch record and the shared species
skeleton were introduced (the parent of the commit that added this file), not from the code under test: a host-side rewrite
of the schedule must leave them as they are.

Names: k_deposit_tiled<order, tile, component mask, laser, valid-by-weight>, k_explicit_tiled<order, derivative type, tile,
laser, pad, valid-by-weight>, k_advance_tiled<order, tile, laser, ionize, valid-by-psi_half, fused deposition's mask>.
The record is process-global: it is switched on and off around each engine's run, one engine at a time."""
import pytest

from hipace_amd import decks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def _blowout(**kw):
    d = decks.blowout_wake()
    d.update(nz=12, n_steps=2, lo=(-8.0, -8.0, -0.72), hi=(8.0, 8.0, 0.72))
    d.update(kw)
    return d


def _laser():
    d = decks.laser_blowout_wake()
    d.update(nx=64, ny=64, nz=24, lo=(-16.0, -16.0, -4.0), hi=(16.0, 16.0, 4.0), laser_a0=1.5, laser_lambda0=0.4, laser_solver=1,
             dt=5.0, n_steps=2)
    return d


def _laser_ionization():      # as test_schedules_do_not_change_results runs it: the tail of released electrons needs the wake
    d = decks.laser_ionization_SI()
    d.update(nx=128, ny=128, nz=60, laser_solver=1, dt=6.0 * 10.0e-6 / 299792458.0, n_steps=2)
    return d


def _predcorr_ion():
    d = decks.predictor_corrector(decks.linear_wake_gaussian(), 4.0e-2, 30, 0.05)
    d.update(nx=64, ny=64, nz=24, plasma_ppc=(2, 2), beam_zmin=d["lo"][2], beam_zmax=d["hi"][2], background_density_SI=1.0e24)
    return decks.with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=0)


# case -> (deck, tile size, sort period, steps, set_fusion).  What each is there for: blowout_16 / _32 the valid-by-weight
# depositions and the valid-by-psi_half push (16 x 16 tiles only); absorbing walls with rho: mask 59, which has no such variant;
# the fused push + deposition; the laser instances, beside a neutralising background that is deposited without |a|^2; the ions'
# IONIZE push under the laser and the electrons' tail; three species; the predictor-corrector's committing (IONIZE) and
# temporary pushes of the ions; SALAME's jx, jy deposits; no tiles: nothing recorded
CASES = {
    "blowout_16": (_blowout, 16, 128, 2, False),
    "blowout_32": (_blowout, 32, 128, 2, False),
    "blowout_absorbing_rho": (lambda: _blowout(bc=2, deposit_rho=1), 16, 128, 2, False),
    "blowout_fused": (_blowout, 16, 128, 2, True),
    "laser": (_laser, 16, 128, 2, False),
    "laser_ionization": (_laser_ionization, 16, 7, 2, False),
    "three_species": (lambda: decks.blowout_wake_three_species(nz=24), 16, 128, 1, False),
    "predcorr_ion": (_predcorr_ion, 16, 128, 1, False),
    "salame": (decks.salame_grid_current, 16, 128, 1, False),      # (100 slices: the witness sits on slices 47 .. 62)
    "untiled": (_blowout, 0, 128, 1, False),
}

EXPECTED = {
    "blowout_16": {"k_advance_tiled<2,16,0,0,1,0>", "k_deposit_tiled<2,16,32,0,0>", "k_deposit_tiled<2,16,51,0,1>",
                   "k_explicit_tiled<2,2,16,0,2,1>"},
    "blowout_32": {"k_advance_tiled<2,32,0,0,0,0>", "k_deposit_tiled<2,32,32,0,0>", "k_deposit_tiled<2,32,51,0,1>",
                   "k_explicit_tiled<2,2,32,0,2,1>"},
    "blowout_absorbing_rho": {"k_advance_tiled<2,16,0,0,1,0>", "k_deposit_tiled<2,16,32,0,0>", "k_deposit_tiled<2,16,59,0,0>",
                              "k_explicit_tiled<2,2,16,0,2,1>"},
    "blowout_fused": {"k_advance_tiled<2,16,0,0,0,51>", "k_advance_tiled<2,16,0,0,1,0>", "k_deposit_tiled<2,16,32,0,0>",
                      "k_deposit_tiled<2,16,51,0,1>", "k_explicit_tiled<2,2,16,0,2,1>"},
    "laser": {"k_advance_tiled<2,16,1,0,1,0>", "k_deposit_tiled<2,16,32,0,0>", "k_deposit_tiled<2,16,51,1,0>",
              "k_explicit_tiled<2,2,16,1,2,0>"},
    "laser_ionization": {"k_advance_tiled<2,16,1,0,1,0>", "k_advance_tiled<2,16,1,1,0,0>", "k_deposit_tiled<2,16,32,0,0>",
                         "k_deposit_tiled<2,16,51,1,0>", "k_explicit_tiled<2,2,16,1,2,0>"},
    "three_species": {"k_advance_tiled<2,16,0,0,0,0>", "k_advance_tiled<2,16,0,0,1,0>", "k_advance_tiled<2,16,0,1,0,0>",
                      "k_deposit_tiled<2,16,59,0,0>", "k_explicit_tiled<2,2,16,0,2,0>", "k_explicit_tiled<2,2,16,0,2,1>"},
    "predcorr_ion": {"k_advance_tiled<2,16,0,0,0,0>", "k_advance_tiled<2,16,0,0,1,0>", "k_advance_tiled<2,16,0,1,0,0>",
                     "k_deposit_tiled<2,16,3,0,0>", "k_deposit_tiled<2,16,3,0,1>", "k_deposit_tiled<2,16,32,0,0>",
                     "k_deposit_tiled<2,16,47,0,0>"},
    "salame": {"k_advance_tiled<2,16,0,0,1,0>", "k_deposit_tiled<2,16,3,0,1>", "k_deposit_tiled<2,16,32,0,0>",
               "k_deposit_tiled<2,16,51,0,1>", "k_explicit_tiled<2,2,16,0,2,1>"},
    "untiled": set(),
}


def run_case(api, name):
    """-> (recorded instances, engine) of one case's run"""
    make, tile, period, steps, fused = CASES[name]
    api.record_particle_dispatch(True)
    try:
        e = api.SliceEngine(make(), tile_size=tile, sort_period=period)
        if fused:
            e.set_fusion(True)
        for _ in range(steps):
            e.run_step()
        e.sync()
        return api.recorded_particle_dispatch(), e
    finally:
        api.record_particle_dispatch(False)


@pytest.mark.parametrize("name", list(CASES))
def test_engine_launches_these_instances(api, name):
    got, e = run_case(api, name)
    if name == "laser_ionization":
        assert e.ion_stats()[0] > 100      # electrons were released: the sheet has a tail behind its sorted body
    assert got == EXPECTED[name], (sorted(got - EXPECTED[name]), sorted(EXPECTED[name] - got))

