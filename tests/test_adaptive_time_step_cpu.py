"""hipace.dt = adaptive without a GPU: the host controller hps_adaptive_* (hipace_amd/csrc/adaptive.hip) against a plain
restatement of the reference's rules (utils/AdaptiveTimeStep.cpp: GatherMinUzSlice, CalculateFromMinUz,
CalculateFromDensity; hipace.max_time in Hipace.cpp:420-435), and the refusals that need no device."""
import math
import sys

import numpy as np
import pytest

from hipace_amd import decks

SI = dict(c=299792458.0, ep0=8.8541878128e-12, q_e=1.602176634e-19, m_e=9.1093837015e-31)


class Restated:
    """The reference's controller, one beam, written out in Python."""

    def __init__(self, d, profile=None):
        self.nt = d["nt_per_betatron"] or 20.0
        self.dt_max = d["dt_max"] or math.inf
        self.thr = d["adaptive_threshold_uz"] or 2.0
        self.tol = d["adaptive_phase_tolerance"] or 4e-4
        self.sub = d["adaptive_phase_substeps"] or 2000
        self.predict = not d["adaptive_no_predict_step"]
        self.phase = not d["adaptive_no_phase_control"]
        self.max_time = d["max_time"] if d["max_time"] != 0.0 else math.inf
        si = bool(d["si_units"])
        self.ep0, self.q_e, self.c = (SI["ep0"], SI["q_e"], SI["c"]) if si else (1.0, 1.0, 1.0)
        self.charge = d["beam_charge"]
        self.mq = (d["beam_mass"] or 1.0) / self.charge if self.charge != 0.0 else 0.0
        self.adens = d["adaptive_density"]
        self.species = []
        if d["plasma_ppc"][0] * d["plasma_ppc"][1] > 0:
            self.species.append(d["plasma_charge"] * d["plasma_density"])
        self.profile = profile
        self.dt = 0.0
        self.min_uz_mq = sys.float_info.max
        self.data = [0.0, 0.0, 0.0, 1e30]

    def _f(self, z):
        if self.profile is None:
            return 1.0
        r, fr, ct, ft = self.profile
        fr0 = float(np.interp(0.0, r, fr)) if len(r) else 1.0
        return fr0 * (float(np.interp(z, ct, ft)) if len(ct) else 1.0)

    def rho(self, z):
        return max([abs(self.adens * self.q_e)] + [abs(q * self._f(z)) for q in self.species])

    def from_min_uz(self, t, nprocs):
        if self.charge == 0.0:
            self.min_uz_mq = sys.float_info.max
            self.dt = min(self.dt, self.dt_max)
            return
        sw, swu, swu2, mn = self.data
        mean = swu / sw
        sigma = math.sqrt(abs(swu2 / sw - mean * mean))
        chosen = max(min(max(mean - 4.0 * sigma, mn), 1e30), self.thr)
        self.min_uz_mq = abs(chosen * self.mq)
        new, time, uz = self.dt, t, chosen
        for _ in range(nprocs if self.predict else 1):
            uz = max(uz, 0.001 * self.thr)
            wb = math.sqrt(self.rho(self.c * time) / (2.0 * abs(uz * self.mq) * self.ep0))
            cand = 2.0 * math.pi / wb / self.nt
            time += cand
            if uz > self.thr:
                new = cand
        self.dt = min(new, self.dt_max)

    def from_density(self, t):
        self.data = [0.0, 0.0, 0.0, 1e30]
        if not self.phase:
            return
        h = self.dt / self.sub
        w0 = math.sqrt(self.rho(self.c * t) / (2.0 * self.min_uz_mq * self.ep0))
        a = a0 = 0.0
        for i in range(self.sub):
            a += math.sqrt(self.rho(self.c * (t + i * h)) / (2.0 * self.min_uz_mq * self.ep0)) * h
            a0 += w0 * h
            if abs(a - a0) > 2.0 * math.pi * self.tol / self.nt:
                self.dt = i * h
                return

    def initial(self, um, us, nprocs):
        self.data = [1.0, um, um * um + us * us, um - 4.0 * us]
        self.from_min_uz(0.0, nprocs)
        self.from_density(0.0)
        return self.dt

    def before(self, t):
        self.from_density(t)
        if t == self.max_time:
            self.dt, nxt = 0.0, math.inf
        elif (t + self.dt >= self.max_time and t < self.max_time) or (t + self.dt <= self.max_time and t > self.max_time):
            self.dt, nxt = self.max_time - t, self.max_time
        else:
            nxt = t + self.dt
        return self.dt, nxt

    def after(self, m, t, nprocs):
        self.data = [self.data[0] + m[0], self.data[1] + m[1], self.data[2] + m[2], min(self.data[3], m[3])]
        self.from_min_uz(t, nprocs)
        return self.dt


def _close(a, b, rtol=1e-14):
    return a == b or abs(a - b) <= rtol * max(abs(a), abs(b))


def _moments(rng, n, mean, spread, w=1.0):
    u = mean + spread * rng.standard_normal(n)
    ww = w * (0.5 + rng.random(n))
    return np.array([ww.sum(), (ww * u).sum(), (ww * u * u).sum(), u.min()])


def _run(deck, nstages, steps, profile=None, seed=0, u0=1000.0, slow_down=0.9, spread=5.0, ustd=0.0):
    """the controller and the restatement side by side over `steps` steps of one stage of `nstages`; -> [(t, dt)], number
    of steps whose dt the phase-advance control cut"""
    from hipace_amd.api import AdaptiveTimeStep
    rng = np.random.default_rng(seed)
    a = AdaptiveTimeStep(deck, profile)
    r = Restated(deck, profile)
    d0 = a.initial_dt(u0, ustd, nstages)
    assert _close(d0, r.initial(u0, ustd, nstages)), (d0, r.dt)
    t, out, u = 0.0, [], u0
    cuts = 0
    for _ in range(steps):
        if t == math.inf:
            break
        planned = r.dt
        dt = a.CalculateFromDensity(t)
        cuts += dt < planned and t != r.max_time      # the phase-advance control has cut this step's dt
        dr, nr = r.before(t)
        assert _close(dt, dr), (t, dt, dr)
        nxt = a.next_time()
        assert nxt == nr or _close(nxt, nr), (nxt, nr)
        out.append((t, dt))
        m = _moments(rng, 50, u, spread)
        got = a.CalculateFromMinUz(m, t, nstages)
        assert _close(got, r.after(m, t, nstages)), (got, r.dt)
        u *= slow_down
        t = nxt
    return out, cuts


def test_initial_estimate_is_the_analysis_value():
    """u_mean = 1000, u_std = 0, density 1 (normalised units): dt = 2 pi sqrt(2 * 1000) / nt_per_betatron (the reference's
    analysis_adaptive_ts.py)"""
    from hipace_amd.api import AdaptiveTimeStep
    d = decks.adaptive_time_step(+1)
    dt = AdaptiveTimeStep(d).initial_dt()
    assert abs(dt - 2 * math.pi * math.sqrt(2 * 1000.0) / 89.7597901025655) <= 1e-14 * dt
    # u_std enters as mean - 4 sigma
    d2 = dict(d, beam_uz_std=10.0)
    want = Restated(d2).initial(1000.0, 10.0, 1)
    assert _close(AdaptiveTimeStep(d2).initial_dt(), want) and want < dt


@pytest.mark.parametrize("nstages", [1, 3])
def test_prediction_over_stages_uniform_density(nstages):
    d = decks.adaptive_time_step(+1)
    out, _ = _run(d, nstages, 8)
    assert len(out) == 8 and all(dt > 0 for _, dt in out)


@pytest.mark.parametrize("nstages", [1, 3])
def test_density_ramp_cuts_dt(nstages):
    """A plasma whose density rises eight-fold along c t (profile table): the phase-advance control cuts dt where the ramp
    starts; the prediction over 3 stages sees the ramp earlier"""
    d = decks.adaptive_time_step(+1)
    d.update(plasma_ppc=(1, 1), plasma_density=1.0, adaptive_density=0.0, adaptive_phase_substeps=400)
    profile = ([0.0, 5.0], [1.0, 0.5], [0.0, 10.0, 100.0], [1.0, 1.0, 8.0])
    out, cuts = _run(d, nstages, 14, profile=profile, slow_down=1.0)
    assert cuts > 0 and out[-1][1] < 0.5 * out[0][1]
    _, cuts = _run(d, nstages, 14, profile=([], [], [0.0, 100.0], [1.0, 1.0]), slow_down=1.0)
    assert cuts == 0                                  # uniform density: nothing to cut


def test_threshold_clamp_and_dt_max():
    d = decks.adaptive_time_step(+1)
    d.update(adaptive_threshold_uz=50.0)
    # the beam slows below the threshold: min uz is clamped to it and dt no longer changes
    out, _ = _run(d, 1, 10, slow_down=0.3, spread=0.0)
    assert out[-1][1] == out[-2][1]
    d.update(adaptive_threshold_uz=0.0, dt_max=3.0)
    out, _ = _run(d, 1, 6)
    assert all(dt <= 3.0 for _, dt in out) and out[1][1] == 3.0


def test_no_phase_control_no_prediction_and_zero_charge():
    d = decks.adaptive_time_step(-1)
    d.update(adaptive_no_predict_step=1, adaptive_no_phase_control=1, plasma_ppc=(1, 1), plasma_density=1.0, adaptive_density=0.0)
    _run(d, 3, 6, profile=([], [], [0.0, 30.0], [1.0, 4.0]))
    d = decks.adaptive_time_step(+1)
    d.update(beam_charge=0.0)
    out, _ = _run(d, 1, 4)
    assert all(dt == 0.0 for _, dt in out)          # the only beam carries no charge: dt stays the deck's 0


def test_si_units():
    """SI: electron mass and charge of the beam, m^-3 densities, u in units of c"""
    ne = 1.0e23
    d = decks.adaptive_time_step(+1)
    d.update(si_units=1, beam_charge=-SI["q_e"], beam_mass=SI["m_e"], plasma_ppc=(1, 1), plasma_density=ne, plasma_charge=-SI["q_e"],
             plasma_mass=SI["m_e"], adaptive_density=0.0, nt_per_betatron=40.0)
    out, _ = _run(d, 3, 6, profile=([], [], [0.0, 0.02, 0.05], [1.0, 1.0, 2.0]))
    wp = math.sqrt(ne * SI["q_e"] ** 2 / (SI["ep0"] * SI["m_e"]))
    assert abs(out[0][1] - 2 * math.pi * math.sqrt(2 * 1000.0) / wp / 40.0) <= 1e-13 * out[0][1]


def test_max_time_clips_and_ends():
    d = decks.adaptive_time_step(+1)
    dt0 = 2 * math.pi * math.sqrt(2 * 1000.0) / 89.7597901025655
    d.update(max_time=2.5 * dt0, adaptive_no_phase_control=1)
    out, _ = _run(d, 1, 10, slow_down=1.0, spread=0.0)
    ts = [t for t, _ in out]
    dts = [dt for _, dt in out]
    assert len(out) == 4                              # t = 0, dt0, 2 dt0 (clipped to 0.5 dt0), max_time (dt = 0)
    assert ts[3] == d["max_time"] and dts[3] == 0.0
    assert _close(dts[2], d["max_time"] - ts[2])


def test_adaptive_deck_with_a_laser_is_refused():
    """Hipace.cpp:408: no laser with the adaptive step -- refused by the engine before it touches a device, and by the
    controller"""
    from hipace_amd import api
    from hipace_amd._lib import HpsError
    d = decks.adaptive_time_step(+1)
    d.update(laser_on=1, laser_a0=1.0)
    with pytest.raises(HpsError, match="laser"):
        api.SliceEngine(d)
    with pytest.raises(HpsError, match="laser"):
        api.AdaptiveTimeStep(d)


def test_adaptive_deck_over_a_ring_of_processes_is_refused():
    """world > 1 (ipc / RCCL / gloo edges) would need the time in the hand-off message: refused, not run with wrong times"""
    from hipace_amd import pipeline

    class Eng:
        deck = decks.adaptive_time_step(+1)
        adaptive = True
        moving = True

    with pytest.raises(NotImplementedError, match="time"):
        next(pipeline._stage(Eng(), 0, 2, 4, "cpu", transport=object()))
    with pytest.raises(NotImplementedError, match="time"):
        pipeline.run_lanes([Eng()], 0, 2, 4, "cpu", transport=object())
