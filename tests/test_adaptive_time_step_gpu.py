"""hipace.dt = adaptive on the GPU: the reference's test (tests/adaptive_time_step.1Rank.sh) pinned by its checksum file and
its analysis script's criteria (examples/beam_in_vacuum/analysis_adaptive_ts.py), the beam moments the partition kernel
reduces (hipace_amd/csrc/beam.hip) against numpy, several steps in flight against one engine fed the same times, and the
fixed-dt path unchanged."""
import json
import math
import os

import numpy as np
import pytest

from hipace_amd import decks

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NT = 89.7597901025655


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()
    return A


def _beam_rows(eng):
    bnd, soa = eng.beam_state()
    return soa[:, bnd[0]:bnd[-1]]


def _run_reference_deck(api, sign, tmp_path=None, keep=None):
    deck = decks.adaptive_time_step(sign)
    eng = api.SliceEngine(deck, tile_size=0)
    eng.set_diagnostics(True)
    if tmp_path is not None:
        eng.set_field_diagnostic(list(json.load(open(os.path.join(GOLD, "adaptive_time_step.1Rank.json")))["lev=0"]))

    def end(step, t, dt):
        if keep is not None and step == deck["n_steps"] - 2:
            keep["beam"] = _beam_rows(eng)

    log = eng.run_adaptive(on_step_end=end)
    return eng, log


def test_adaptive_time_step_matches_reference_checksums(api, tmp_path):
    """the +0.5 z run of tests/adaptive_time_step.1Rank.sh (21 adaptive steps): field checksums of the last step and the beam
    block through the openPMD writer and the checksum backend's reductions, against the reference's file"""
    from hipace_amd import openpmd_writer as W
    from tests import openpmd_shim as S
    gold = json.load(open(os.path.join(GOLD, "adaptive_time_step.1Rank.json")))
    keep = {}
    eng, log = _run_reference_deck(api, +1, tmp_path, keep)
    assert [s for s, _, _ in log] == list(range(21))
    cs = eng.checksums()
    for k, v in gold["lev=0"].items():
        if v == 0.0:
            assert cs[k] == 0.0, (k, cs[k])
        else:
            assert abs(cs[k] - v) <= 1e-9 * abs(v), (k, cs[k], v)
    # the reference copies the beam for its diagnostic before the slice's push (FillBeamDiagnostics, Hipace.cpp:680-682):
    # the beam of the last step's output is the beam the step began with
    step, t, dt = log[-1]
    W.write_engine_output(eng, str(tmp_path), step, time=t, beam=keep["beam"])
    got = S.checksums(str(tmp_path))
    for grp in ("lev=0", "beam"):
        for k, v in gold[grp].items():
            if v == 0.0:
                assert got[grp][k] == 0.0, (grp, k, got[grp][k])
            else:
                assert abs(got[grp][k] - v) <= 1e-9 * abs(v), (grp, k, got[grp][k], v)


def test_adaptive_time_step_analysis_criteria(api):
    """analysis_adaptive_ts.py on the dt sequences of the +0.5 z and -0.5 z runs"""
    _, lp = _run_reference_deck(api, +1)
    _, ln = _run_reference_deck(api, -1)
    dt1 = np.array([dt for _, _, dt in lp])
    dt2 = np.array([dt for _, _, dt in ln])
    analytic = math.sqrt(2 * 1000.0) / NT * 2 * math.pi
    assert abs(dt1[0] - analytic) / analytic < 1e-5
    assert abs(np.sum(dt1 - dt2)) / np.sum(dt2) < 1e-6
    assert all(dt2[i + 1] > dt2[i + 2] for i in range(len(dt2) - 2))
    assert not np.array_equal(dt1, dt2)           # the two runs do differ step by step
    # the times chain: each step starts where the last one ended
    ts = [t for _, t, _ in lp]
    assert ts[0] == 0.0 and all(ts[k + 1] == ts[k] + dt1[k] for k in range(len(ts) - 1))


def _hot_beam_deck():
    """test_beam_slipping_matches_oracle's slow, hot beam (u_z = 1.2), slipping through several slices per step, in an
    absorbing box with a strongly defocusing field: particles leave the box transversely (absorbed) and through the tail"""
    deck = decks.beam_evolution()
    deck.update(nz=12, lo=(-2.0, -2.0, -2.4), hi=(2.0, 2.0, 2.4), beam_zmin=-1.0, beam_zmax=1.6, beam_umean=(0.0, 0.0, 1.2),
                beam_density=1.0e-3, beam_radius=1.9, n_steps=3, dt=4.0, beam_n_subcycles=16, ext_E_slope=(-2.0, -1.5),
                ext_Ez_slope=0.2, bc=2, dt_adaptive=1, adaptive_density=1.0)
    return deck


def _numpy_moments(eng):
    bnd, soa = eng.beam_state()
    z, uz, w = soa[2], soa[5], soa[6]
    sel = np.zeros(soa.shape[1], dtype=bool)
    sel[bnd[0]:bnd[-1]] = True
    sel &= w != 0.0                                    # absorbed particles have w = 0 (and nsub < 0)
    u = uz[sel]
    return np.array([w[sel].sum(), (w[sel] * u).sum(), (w[sel] * u * u).sum(), u.min() if u.size else np.inf]), soa, bnd


def _hot_run(api):
    deck = _hot_beam_deck()
    eng = api.SliceEngine(deck, tile_size=0)
    n0 = eng.beam_layout()[0]
    out = []
    for s in range(deck["n_steps"]):
        eng.set_time(s * 4.0, 4.0)
        eng.run_step()
        m = eng.beam_moments()
        want, soa, bnd = _numpy_moments(eng)
        out.append((m, want, soa, bnd))
    return n0, out


def test_beam_moments_match_numpy(api):
    n0, out = _hot_run(api)
    for m, want, soa, bnd in out:
        for k in range(3):
            assert abs(m[k] - want[k]) <= 1e-13 * abs(want[k]), (k, m[k], want[k])
        assert m[3] == want[3]
    absorbed = int(np.sum(soa[6] == 0.0))
    left = n0 - (bnd[-1] - bnd[0])
    assert absorbed > 0 and left > 0                  # the deck does absorb particles and lose some through the tail


def test_beam_moments_are_bit_reproducible(api):
    """equal inputs, bit-identical moments (a fixed lane-to-particle mapping and a fixed reduction tree): after the hot beam's
    steps -- particles slipped, absorbed, gone through the tail -- two steps of dt = 0 reduce the same particles in the same
    order twice (nothing moves, nothing slips): the moments agree to the bit, and with numpy"""
    deck = _hot_beam_deck()
    eng = api.SliceEngine(deck, tile_size=0)
    for s in range(deck["n_steps"]):
        eng.set_time(s * 4.0, 4.0)
        eng.run_step()
    moms, states = [], []
    for _ in range(2):
        eng.set_time(deck["n_steps"] * 4.0, 0.0)
        eng.run_step()
        moms.append(eng.beam_moments())
        states.append(eng.beam_state())
    assert np.array_equal(states[0][0], states[1][0]) and states[0][1].tobytes() == states[1][1].tobytes()
    assert moms[0].tobytes() == moms[1].tobytes()
    want = _numpy_moments(eng)[0]
    assert all(abs(moms[0][k] - want[k]) <= 1e-13 * abs(want[k]) for k in range(3)) and moms[0][3] == want[3]


def test_beam_moments_of_an_empty_step_and_refusals(api):
    deck = decks.adaptive_time_step(+1)
    eng = api.SliceEngine(dict(deck, beam_profile=-1))
    with pytest.raises(RuntimeError, match="beam"):
        eng.begin_step()
    eng = api.SliceEngine(dict(deck, beam_profile=-1, n_steps=1))
    assert eng.set_beam_particles(np.zeros((7, 0))) == 0
    eng.run_step()
    m = eng.beam_moments()
    assert m[0] == 0.0 and m[1] == 0.0 and m[2] == 0.0 and m[3] == np.inf
    fixed = api.SliceEngine(decks.beam_evolution(), tile_size=0)
    with pytest.raises(RuntimeError, match="adaptive"):
        fixed.beam_moments()


@pytest.mark.parametrize("L", [2, 3])
def test_steps_in_flight_follow_the_rule_and_match_one_engine(api, L):
    """run_local_pipeline with L stages on the reference deck: each stage's (t, dt) follows the controller with nstages = L,
    and the last step equals one engine fed the same (t, dt) sequence through set_time"""
    import torch
    from hipace_amd.api import AdaptiveTimeStep
    from hipace_amd.pipeline import run_local_pipeline
    deck = decks.adaptive_time_step(+1)
    n = deck["n_steps"]
    engines = [api.SliceEngine(deck, tile_size=0) for _ in range(L)]
    for e in engines:
        e.set_diagnostics(True)
    last = {}

    def on_end(step, e):
        if step == n - 1:
            e.sync()
            last["cs"] = e.checksums()
            last["beam"] = e.beam_state()

    run_local_pipeline(engines, n, torch.device("cuda", 0), on_step_end=on_end)
    seq = sorted(x for e in engines for x in e.step_times)
    assert [s for s, _, _ in seq] == list(range(n))
    for j, e in enumerate(engines):
        assert [s for s, _, _ in e.step_times] == list(range(j, n, L))
    dt0 = AdaptiveTimeStep(deck).initial_dt(nstages=L)
    assert all(dt == dt0 for s, _, dt in seq[:L])          # every stage starts with the broadcast dt
    assert all(seq[k + 1][1] == seq[k][1] + seq[k][2] for k in range(n - 1))
    # the rule, stage by stage: replay each stage's controller on moments of a single engine fed the same times
    ref = api.SliceEngine(deck, tile_size=0)
    ref.set_diagnostics(True)
    ctl = [AdaptiveTimeStep(deck) for _ in range(L)]
    for c in ctl:
        c.initial_dt(nstages=L)
    for s, t, dt in seq:
        c = ctl[s % L]
        got = c.CalculateFromDensity(t)
        assert abs(got - dt) <= 1e-12 * dt, (s, t, got, dt)
        ref.set_time(t, dt)
        ref.run_step()
        c.CalculateFromMinUz(ref.beam_moments(), t, L)
    cs = ref.checksums()
    for k, v in last["cs"].items():
        assert abs(cs[k] - v) <= 1e-12 * max(abs(v), 1e-300), (k, cs[k], v)
    bnd, soa = ref.beam_state()
    gb, gs = last["beam"]
    nz = deck["nz"]
    for p in range(nz):
        want = soa[:, bnd[p]:bnd[p + 1]]
        got = gs[:, gb[p]:gb[p + 1]]
        assert got.shape == want.shape, p
        if want.shape[1]:
            ko = np.lexsort((want[1], want[0])); kg = np.lexsort((got[1], got[0]))
            assert np.abs(got[:, kg] - want[:, ko]).max() <= 1e-12 * np.abs(want).max()


def _fixed_run(api, deck, via_set_time):
    e = api.SliceEngine(deck, tile_size=0)
    e.set_diagnostics(True)
    for s in range(deck["n_steps"]):
        if via_set_time:
            e.set_time(s * deck["dt"], deck["dt"])
        e.run_step()
    return e.checksums(), e.beam_state()


def test_fixed_dt_results_unchanged_by_set_time(api):
    """beam_evolution (fixed dt = 3) as before and through set_time(step * dt, dt).  A beam without charge has fields that
    are exactly zero, so its runs are reproducible to the bit: there the two agree to the bit.  With the charge the
    deposition's atomics make two runs differ in the last bits (two plain runs are compared too): there the two agree as
    closely as two plain runs do."""
    deck = decks.beam_evolution()
    neutral = dict(deck, beam_charge=0.0)
    (ca, (ba, sa)), (cb, (bb, sb)) = _fixed_run(api, neutral, False), _fixed_run(api, neutral, True)
    assert all(ca[k] == cb[k] for k in ca) and np.array_equal(ba, bb) and sa.tobytes() == sb.tobytes()
    assert np.any(sa[2] != _fixed_run(api, dict(neutral, n_steps=1), False)[1][1][2])       # z did move (free streaming at dt = 3)
    (ca, (ba, sa)), (cb, (bb, sb)), (cc, (bc, sc)) = (_fixed_run(api, deck, False), _fixed_run(api, deck, True),
                                                      _fixed_run(api, deck, False))
    spread = max([abs(ca[k] - cc[k]) / max(abs(ca[k]), 1e-300) for k in ca] + [0.0])
    for k in ca:
        assert abs(cb[k] - ca[k]) <= max(1e-13, 10 * spread) * max(abs(ca[k]), 1e-300), (k, ca[k], cb[k])
    assert np.array_equal(ba, bb)
    assert np.abs(sb - sa).max() <= 1e-13 * np.abs(sa).max()
    if sa.tobytes() == sc.tobytes() and all(ca[k] == cc[k] for k in ca):
        assert sa.tobytes() == sb.tobytes() and all(ca[k] == cb[k] for k in ca)
