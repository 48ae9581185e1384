"""numpy restatement of the sub-cycled beam push of the reference (AdvanceBeamParticlesSlice,
particles/pusher/BeamParticleAdvance.cpp:20-336) for a beam in vacuum: no gather -- every grid field is exactly zero -- so
the only fields are beams.external_E / external_B (ApplyExternalField, particles/pusher/ExternalFields.H:29-56), taken from
hipace_amd.expr.Program.evaluate, plus the deck's ext_E_slope / ext_Ez_slope.  Covered: the position half-steps, the
particle boundary (EnforceBC), the momentum update, radiation reaction, spin, the slice-exit rule z < min_z with the
hand-over of slipped particles to the next slice (shiftSlippedParticles), which finish their sub-cycles there.

State: one row per particle in input order, so a test can follow every particle: `islice` is the slice it sits on (-1: it
left the box through the tail), `alive` is False once it was absorbed at the wall -- such a particle keeps the state it had
when the push of the slice that absorbed it began, as the engine's arrays do."""
import numpy as np

from hipace_amd import expr

C_SI, QE_SI, ME_SI, EP0_SI, RE_SI = 299792458.0, 1.602176634e-19, 9.1093837015e-31, 8.8541878128e-12, 2.817940326204929e-15


def compile_fields(E=None, B=None, constants=None):
    """-> six Programs or None (absent / constant 0), order Ex Ey Ez Bx By Bz"""
    out = []
    for three, what in ((E, "E"), (B, "B")):
        progs = expr.compile_components(three, what, constants) or [None] * 3
        out += [None if (p is None or p.is_zero) else p for p in progs]
    return out


class BeamRestatement:
    def __init__(self, deck, soa, fields=None, spin=None):
        """soa: (7, n) x y z ux uy uz w, all inside the box in z; fields: compile_fields(...)"""
        self.d = dict(deck)
        d = self.d
        soa = np.array(soa, dtype=np.float64)
        self.x, self.y, self.z, self.ux, self.uy, self.uz, self.w = [soa[k].copy() for k in range(7)]
        n = soa.shape[1]
        self.nz = d["nz"]
        self.dz = (d["hi"][2] - d["lo"][2]) / d["nz"]
        self.islice = ((self.z - d["lo"][2]) / self.dz).astype(np.int64)      # BoxSorter: int((z - lo)/dz)
        assert np.all((self.islice >= 0) & (self.islice < self.nz))
        self.alive = np.ones(n, dtype=bool)
        self.fields = fields or [None] * 6
        self.spin_on = bool(d.get("beam_spin_tracking", 0))
        s0 = d.get("beam_initial_spin", (1.0, 0.0, 0.0))
        self.s = np.array(spin, dtype=np.float64) if spin is not None else np.repeat(np.array(s0, dtype=np.float64)[:, None], n, axis=1)
        self.step = 0
        self.n_slipped_mid_step = 0      # hand-overs of particles that still had sub-cycles to do
        self.n_absorbed = 0

    # EnforceBC (particles/pusher/GetAndSetPosition.H:29-99) on the rows `m`; -> mask of the rows absorbed
    def _bc(self, x, y, ux, uy):
        d = self.d
        lo0, lo1, hi0, hi1 = d["lo"][0], d["lo"][1], d["hi"][0], d["hi"][1]
        out = (x < lo0) | (y < lo1) | (x > hi0) | (y > hi1)
        gone = np.zeros(x.shape, dtype=bool)
        if not out.any():
            return gone
        lx, ly = hi0 - lo0, hi1 - lo1
        bc = d.get("bc", 1)
        if bc == 0:      # reflecting
            xn = np.fmod(x - lo0, 2 * lx); xn = np.where(xn < 0, xn + 2 * lx, xn) + lo0
            fx = xn > hi0
            xn = np.where(fx, 2 * hi0 - xn, xn)
            yn = np.fmod(y - lo1, 2 * ly); yn = np.where(yn < 0, yn + 2 * ly, yn) + lo1
            fy = yn > hi1
            yn = np.where(fy, 2 * hi1 - yn, yn)
            x[out], y[out] = xn[out], yn[out]
            ux[out & fx] = -ux[out & fx]
            uy[out & fy] = -uy[out & fy]
        elif bc == 1:    # periodic
            xn = np.fmod(x - lo0, lx); xn = np.where(xn < 0, xn + lx, xn) + lo0
            yn = np.fmod(y - lo1, ly); yn = np.where(yn < 0, yn + ly, yn) + lo1
            x[out], y[out] = xn[out], yn[out]
        else:            # absorbing
            gone = out
        return gone

    def _push_slice(self, islice, t, dt_step):
        d = self.d
        sel = np.flatnonzero(self.alive & (self.islice == islice))
        if sel.size == 0:
            return
        nsc = d.get("beam_n_subcycles", 10) or 10
        dt = dt_step / nsc
        c = 1.0 if not d.get("si_units", 0) else C_SI
        inv_c2 = 1.0 / (c * c)
        mass = d.get("beam_mass", 1.0) or 1.0
        qm = d["beam_charge"] / mass
        min_z = d["lo"][2] + islice * self.dz
        sx_, sy_ = d.get("ext_E_slope", (0.0, 0.0))
        sz_ = d.get("ext_Ez_slope", 0.0)
        rr = bool(d.get("beam_radiation_reaction", 0))
        normalized = not d.get("si_units", 0)
        if rr:
            q_over_mc = qm / C_SI * QE_SI / ME_SI if normalized else qm / C_SI
            RRcoeff = (2.0 / 3.0) * RE_SI * q_over_mc * q_over_mc
            wp_inv = np.sqrt(EP0_SI * ME_SI / (d["background_density_SI"] * QE_SI * QE_SI)) if normalized else 1.0
            E0 = ME_SI * C_SI / wp_inv / QE_SI if normalized else 1.0
        anom = d.get("beam_spin_anom", 0.0)
        x, y, z = self.x[sel].copy(), self.y[sel].copy(), self.z[sel].copy()
        ux, uy, uz = self.ux[sel].copy(), self.uy[sel].copy(), self.uz[sel].copy()
        s = self.s[:, sel].copy()
        nsub = self.nsub[sel].copy()
        absorbed = np.zeros(sel.size, dtype=bool)
        left = np.zeros(sel.size, dtype=bool)          # broke out of the loop: z < min_z
        for _ in range(nsc):
            left |= ~absorbed & (nsub < nsc) & (z < min_z)
            a = np.flatnonzero(~absorbed & ~left & (nsub < nsc))
            if a.size == 0:
                break
            xp, yp, zp, uxp, uyp, uzp = x[a], y[a], z[a], ux[a], uy[a], uz[a]
            gi = 1.0 / np.sqrt(1.0 + (uxp * uxp + uyp * uyp + uzp * uzp) * inv_c2)
            xp = xp + dt * 0.5 * uxp * gi
            yp = yp + dt * 0.5 * uyp * gi
            gone = self._bc(xp, yp, uxp, uyp)
            tt = np.full(xp.shape, t)
            f = [np.zeros(xp.shape) if p is None else p.evaluate(xp, yp, zp, tt) for p in self.fields]
            ExmBy = np.zeros(xp.shape) + sx_ * xp
            EypBx = np.zeros(xp.shape) + sy_ * yp
            Ez = np.zeros(xp.shape) + (sz_ * zp if sz_ != 0.0 else 0.0)
            ExmBy = ExmBy + (f[0] - c * f[4])
            EypBx = EypBx + (f[1] + c * f[3])
            Ez = Ez + f[2]
            Bx, By, Bz = f[3], f[4], f[5]
            ux_n = uxp + dt * qm * (ExmBy + (c - uzp * gi) * By + uyp * gi * Bz)
            uy_n = uyp + dt * qm * (EypBx + (uzp * gi - c) * Bx - uxp * gi * Bz)
            ux_i, uy_i = (ux_n + uxp) * 0.5, (uy_n + uyp) * 0.5
            uz_i = uzp + dt * 0.5 * qm * Ez
            gii = 1.0 / np.sqrt(1.0 + (ux_i * ux_i + uy_i * uy_i + uz_i * uz_i) * inv_c2)
            if self.spin_on:      # Thomas-BMT precession as a Boris-type rotation (:218-238)
                ic = 1.0 / c
                Ev = np.array([ExmBy + c * By, EypBx - c * Bx, Ez])
                Bv = np.array([Bx, By, Bz])
                u = np.array([ux_i * ic, uy_i * ic, uz_i * ic])
                be = u * gii
                gp1 = gii / (1.0 + gii)
                bxE = np.cross(be, Ev, axis=0)
                bdB = (be * Bv).sum(axis=0)
                h = abs(qm) * (Bv * gii - bxE * ic * gp1 + anom * (Bv - gp1 * u * bdB - bxE * ic)) * dt * 0.5
                sa = s[:, a]
                sp = sa + np.cross(h, sa, axis=0)
                o = 1.0 / (1.0 + (h * h).sum(axis=0))
                hd = (h * sp).sum(axis=0)
                sa = o * (sp + (hd * h + np.cross(h, sp, axis=0)))
            uz_n = uzp + dt * qm * (Ez + (ux_i * By - uy_i * Bx) * gii)
            if rr:                # classical radiation reaction in SI quantities (:244-297)
                icSI, ic = 1.0 / C_SI, 1.0 / c
                Ex, Ey, Ezs, Bxs, Bys, Bzs = ExmBy + c * By, EypBx - c * Bx, Ez, Bx, By, Bz
                if normalized:
                    Ex, Ey, Ezs = Ex * E0, Ey * E0, Ezs * E0
                    Bxs, Bys, Bzs = Bxs * (E0 * icSI), Bys * (E0 * icSI), Bzs * (E0 * icSI)
                gam = np.sqrt(1.0 + (ux_i * ux_i + uy_i * uy_i + uz_i * uz_i) * inv_c2)
                vx, vy, vz = ux_i * gii * C_SI * ic, uy_i * gii * C_SI * ic, uz_i * gii * C_SI * ic
                bx, by, bz = vx * icSI, vy * icSI, vz * icSI
                flx, fly, flz = Ex + vy * Bzs - vz * Bys, Ey + vz * Bxs - vx * Bzs, Ezs + vx * Bys - vy * Bxs
                fl2 = flx * flx + fly * fly + flz * flz
                bE = bx * Ex + by * Ey + bz * Ezs
                coeff = gam * gam * (fl2 - bE * bE)
                frx = RRcoeff * (C_SI * (fly * Bzs - flz * Bys) + bE * Ex - coeff * bx)
                fry = RRcoeff * (C_SI * (flz * Bxs - flx * Bzs) + bE * Ey - coeff * by)
                frz = RRcoeff * (C_SI * (flx * Bys - fly * Bxs) + bE * Ezs - coeff * bz)
                sc = dt * wp_inv * c * icSI
                ux_n, uy_n, uz_n = ux_n + frx * sc, uy_n + fry * sc, uz_n + frz * sc
            gni = 1.0 / np.sqrt(1.0 + (ux_n * ux_n + uy_n * uy_n + uz_n * uz_n) * inv_c2)
            xp = xp + dt * 0.5 * ux_n * gni
            yp = yp + dt * 0.5 * uy_n * gni
            if not d.get("beam_no_z_push", 0):
                zp = zp + dt * (uz_n * gni - c)
            keep = ~gone                    # an absorbed particle stops at the boundary check: nothing of this sub-step is kept
            k = a[keep]
            x[k], y[k], z[k], ux[k], uy[k], uz[k] = xp[keep], yp[keep], zp[keep], ux_n[keep], uy_n[keep], uz_n[keep]
            if self.spin_on:
                s[:, k] = sa[:, keep]
            nsub[k] += 1
            absorbed[a[gone]] = True
        absorbed |= ~absorbed & self._bc(x, y, ux, uy)      # the check behind the loop (:323)
        ok = ~absorbed
        w = sel[ok]
        self.x[w], self.y[w], self.z[w], self.ux[w], self.uy[w], self.uz[w] = x[ok], y[ok], z[ok], ux[ok], uy[ok], uz[ok]
        self.s[:, w] = s[:, ok]
        self.nsub[w] = nsub[ok]
        self.alive[sel[absorbed]] = False
        self.n_absorbed += int(absorbed.sum())
        # shiftSlippedParticles: z < min_z goes to the next slice (and is pushed again there if sub-cycles are left)
        slip = w[self.z[w] < min_z]
        self.n_slipped_mid_step += int((self.nsub[slip] < nsc).sum())
        self.islice[slip] = islice - 1

    def run_step(self, t=None, dt=None):
        """one time step: t = the step's physical time (default dt*step), dt = its length (default the deck's)"""
        d = self.d
        dt_step = d["dt"] if dt is None else dt
        t = d["dt"] * self.step if t is None else t
        self.nsub = np.zeros(self.x.size, dtype=np.int64)
        for islice in range(self.nz - 1, -1, -1):
            self._push_slice(islice, t, dt_step)
        self.step += 1

    def state(self):
        """-> (7, n) x y z ux uy uz w in input order"""
        return np.array([self.x, self.y, self.z, self.ux, self.uy, self.uz, self.w])


def match_engine_state(bnd, soa, ref, spin=None):
    """the engine's beam_state() (boundaries, soa[7, n]) brought into the restatement's particle order: per slice the
    particles sorted by (x, y), on both sides.  -> (soa in ref order, spin in ref order or None); asserts that every slice
    holds as many particles as the restatement says (absorbed particles stay on their slice, particles that left through
    the tail are in no slice)."""
    nz = ref.nz
    n = ref.x.size
    out = np.full((7, n), np.nan)
    sout = np.full((3, n), np.nan) if spin is not None else None
    for p in range(nz):
        isl = nz - 1 - p
        idx = np.flatnonzero(ref.islice == isl)
        got = soa[:, bnd[p]:bnd[p + 1]]
        assert got.shape[1] == idx.size, (isl, got.shape[1], idx.size)
        if idx.size == 0:
            continue
        ko = np.lexsort((ref.y[idx], ref.x[idx]))
        kg = np.lexsort((got[1], got[0]))
        out[:, idx[ko]] = got[:, kg]
        if spin is not None:
            sout[:, idx[ko]] = spin[:, bnd[p]:bnd[p + 1]][:, kg]
    return out, sout


# ---- the shared vacuum case of tests/test_external_fields_cpu.py and tests/test_external_fields_gpu.py -----------------
FIELDS_E = ("0.3*x + 0.05*y*t", "if(z > -0.2, 0.2*y, -0.1*y)", "0.1*z - 0.02*t")
FIELDS_B = ("0.4*y", "0.4*x", "0.05")
LINEAR_SLOPES = (0.3, 0.2, 0.1)      # the deck-slope path's field of like size: E = (0.3 x, 0.2 y, 0.1 z)


def vacuum_deck(order=2, spin=False, rr=False, bc=2):
    """32 x 32 cells, 12 slices of dz = 0.4, no plasma, 3 steps of dt = 0.9 in 4 sub-cycles, absorbing walls"""
    from hipace_amd import decks
    d = decks.beam_evolution()
    d.update(decks.ADAPTIVE_DEFAULT)
    d.update(nx=32, ny=32, nz=12, lo=(-2.0, -2.0, -2.4), hi=(2.0, 2.0, 2.4), order=order, plasma_ppc=(0, 0), plasma_density=0.0,
             beam_profile=-1, n_steps=3, dt=0.9, beam_n_subcycles=4, ext_E_slope=(0.0, 0.0), ext_Ez_slope=0.0, bc=bc,
             beam_spin_tracking=int(spin), beam_initial_spin=(0.6, 0.0, 0.8), beam_radiation_reaction=int(rr),
             background_density_SI=1.0e23 if rr else 0.0)
    return d


def vacuum_beam(n=333):
    """(7, n) host beam of weight exactly 0: more than one 256-lane workgroup, not a multiple of 64.  Fast particles
    (u_z = 30) everywhere but on slices 4 and 11, which start empty; particles 0 .. 4 are slow (u_z = 1.2,
    v_z = 0.77 c: 0.21 per step backwards) and sit just above the lower end of their slice, so they slip in mid-step;
    particle 5 starts next to the wall x = 2 and moves outwards."""
    rng = np.random.default_rng(20)
    soa = np.zeros((7, n))
    soa[0] = rng.uniform(-1.2, 1.2, n)
    soa[1] = rng.uniform(-1.2, 1.2, n)
    z = rng.uniform(-2.4 + 0.05, 2.0 - 0.05, n)     # the head slice 11 (z in [2.0, 2.4)) stays empty: nothing is launched for it
    on4 = (z >= -2.4 + 4 * 0.4) & (z < -2.4 + 5 * 0.4)
    z[on4] += 0.4                                   # slice 4 (z in [-0.8, -0.4)) starts empty: launched with a count of 0
    soa[2] = z
    soa[3] = rng.normal(0.0, 0.5, n)
    soa[4] = rng.normal(0.0, 0.5, n)
    soa[5] = 30.0 + rng.normal(0.0, 1.0, n)
    for k in range(5):                              # the slow ones: 0.03 .. 0.15 above the lower end of slices 6 .. 10
        soa[2, k] = -2.4 + (6 + k) * 0.4 + 0.03 * (k + 1)
        soa[5, k] = 1.2
        soa[3, k], soa[4, k] = 0.1 * (k - 2), -0.05 * k
    soa[0, 5], soa[3, 5], soa[2, 5] = 1.9, 25.0, 1.0      # v_x = 0.64 c outwards: through the wall in the first step
    return soa
