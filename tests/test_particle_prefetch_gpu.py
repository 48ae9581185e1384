"""The record pipelines of k_explicit_tiled and k_advance_tiled (particles_tiled.hip): thread t of a tile's workgroup works on
the records first + t + 256 m, requests record m + 1 while it works on record m, and -- in the push -- holds particle m's
stores back until record m + 1 has arrived.  The cases sit where such a pipeline can go wrong, each against the oracle at
the tolerances of tests/test_particle_dispatch_gpu.py (explicit deposition 1e-12 of the deposited sources, push 1e-10 per
particle quantity; validity flags and the fallback counter exact):

  * tile populations 1, 255, 256, 257, 511, 512, 513, 769: threads of one workgroup with 0, 1, 2, 3 and 4 records, the first
    and the last record of a thread's sequence on the boundaries -- on a 48 x 32 grid and on a 17 x 9 grid (smaller than one
    tile), order 2 and one of orders 0 / 3, 16 x 16 and 32 x 32 tiles;
  * invalid records (w = 0, psi_half = 0, valid bit clear: Tiling.set_validity) at positions 256 k - 1, 256 k, 256 k + 1 of a
    tile -- the first or last record of a thread, or the one requested behind a valid one -- and a tile without a valid record;
  * the push with 1, 2, 3 sub-cycles and temp_slice 0 / 1 under the absorbing boundary, with particles that leave in the
    first and in a later sub-cycle;
  * a stale sort: one particle per workgroup, and several consecutive records of one thread, far outside their tile's
    image (the slab path of the push, the second pass of the explicit deposition); and the workgroups of the particles
    appended behind the sorted body, which only an ionising engine has."""
import numpy as np
import pytest

from hipace_amd import decks
from tests.util import NCOMP, rel_err, smooth_slab

pytestmark = pytest.mark.gpu

LO, HI = (-8.0, -8.0), (8.0, 8.0)
CACHE, SRC = [10, 7, 5, 6], [3, 4]           # Bz Ez ExmBy EypBx -> Sy Sx
PUSH = [11, 7, 8, 9, 10]                     # Psi Ez Bx By Bz
POPS = (1, 255, 256, 257, 511, 512, 513, 769)
HALO = 6


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


class Sheet:
    """A sheet with a prescribed number of particles in every tile, tile-sorted on the device; every particle sits in the
    inner 80 % of a cell of its tile, so its stencil lies inside the tile's image at every order."""

    def __init__(self, api, oracle, nx, ny, ts, order, pops, seed, bc=1, dz=0.3):
        rng = np.random.default_rng(seed)
        self.nx, self.ny, self.ts, self.g = nx, ny, ts, (order + 1) // 2 + 1
        self.dx, self.dy = (HI[0] - LO[0]) / nx, (HI[1] - LO[1]) / ny
        self.geom = api.Geometry(nx, ny, LO, HI, dz, bc=bc)
        self.ogeom = oracle.make_geom(nx, ny, LO, HI, dz=dz, bc=bc)
        self.ntx, self.nty = (nx + ts - 1) // ts, (ny + ts - 1) // ts
        nt = self.ntx * self.nty
        self.pops = np.array([pops[t % len(pops)] for t in range(nt)])
        ci, cj = [], []
        for t, p in enumerate(self.pops):
            i0, j0 = (t % self.ntx) * ts, (t // self.ntx) * ts
            ci.append(rng.integers(i0, min(i0 + ts, nx), p))
            cj.append(rng.integers(j0, min(j0 + ts, ny), p))
        ci, cj = np.concatenate(ci), np.concatenate(cj)
        n = ci.size
        shuffle = rng.permutation(n)                  # the sort has work to do
        ci, cj = ci[shuffle], cj[shuffle]
        x = LO[0] + (ci + 0.5 + 0.8 * (rng.random(n) - 0.5)) * self.dx
        y = LO[1] + (cj + 0.5 + 0.8 * (rng.random(n) - 0.5)) * self.dy
        ux, uy, uz = rng.normal(0.0, 0.3, (3, n))
        psi = np.sqrt(1.0 + ux * ux + uy * uy + uz * uz) - uz
        real = np.empty((11, n))
        real[0], real[1], real[2], real[3], real[4], real[5] = x, y, 0.5 + rng.random(n), ux, uy, psi
        real[6], real[7] = x, y
        real[8], real[9] = ux + rng.normal(0.0, 0.01, n), uy + rng.normal(0.0, 0.01, n)
        real[10] = psi * (1.0 + rng.normal(0.0, 0.01, n))
        self.ion = np.zeros(n, dtype=np.int32)
        self.til = api.Tiling(nx, ny, ts, n)
        sheet = self.til.reorder(api.PlasmaSheet(real, np.ones(n, dtype=np.int32), self.ion), self.geom)
        r, v = sheet.numpy()
        off, _ = self.til.offsets_and_perm(n)
        self.first = off[:nt].astype(np.int64)
        assert np.array_equal(np.diff(off[:nt + 1]), self.pops), "the sort did not give the prescribed tile populations"
        self.real, self.valid, self.n = r, v.astype(np.int32), n
        self.slab = smooth_slab(nx, ny, self.g, amp=0.2)

    def record(self, tile, pos):
        """Index in the sorted sheet of record `pos` of `tile`."""
        assert 0 <= pos < self.pops[tile]
        return int(self.first[tile] + pos)

    def invalidate(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        self.valid[idx] = 0
        self.real[2, idx] = 0.0
        self.real[10, idx] = 0.0

    def move_far(self, tile, idx):
        """Puts the records idx of `tile` 3 or more cells beyond the tile's image, without re-sorting."""
        ox = (tile % self.ntx) * self.ts
        ci = ox + self.ts + HALO + 3
        if ci > self.nx - 1:
            ci = ox - HALO - 4
        assert 0 <= ci < self.nx and max(self.nx, self.ny) > self.ts + 2 * HALO
        idx = np.asarray(idx, dtype=np.int64)
        self.real[0, idx] = LO[0] + (ci + 0.5) * self.dx + 0.1 * self.dx * np.arange(idx.size) / max(idx.size, 1)
        self.real[6, idx] = self.real[0, idx]

    def sheet(self, api):
        return api.PlasmaSheet(self.real, self.valid, self.ion)


def _explicit(api, oracle, S, order, vbw, expect_fallback):
    import torch
    S.til.set_validity(by_weight=vbw)
    pl, f = S.sheet(api), api.Fields(S.nx, S.ny, S.g, NCOMP, data=S.slab)
    S.til.fallback.zero_()
    api.ExplicitDeposition(pl, f, S.geom, -1.0, 1.0, order, *CACHE, *SRC, derivative_type=2, tiling=S.til)
    torch.cuda.synchronize()
    out = f.numpy()
    o = S.slab.copy()
    oracle.explicit_deposit(o, S.nx, S.ny, S.g, S.real.copy(), S.valid.copy(), S.ion, S.ogeom, CACHE, SRC, -1.0, 1.0, order, 2)
    for c in SRC:
        if S.valid.any():
            err = rel_err(out[c] - S.slab[c], o[c] - S.slab[c])
            assert err < 1e-12, (c, err)
        else:
            assert np.array_equal(out[c], S.slab[c]) and np.array_equal(o[c], S.slab[c])
    rest = [c for c in range(NCOMP) if c not in SRC]
    assert np.array_equal(out[rest], S.slab[rest]), "a component that is not a source was written"
    assert S.til.fallback.item() == expect_fallback
    r, v = pl.numpy()
    assert np.array_equal(r, S.real) and np.array_equal(v, S.valid), "the deposition wrote to the sheet"


def _push(api, oracle, S, order, vbp, nsub=1, temp=0, expect_fallback=0):
    """-> (oracle's sheet, oracle's flags) after the push, compared with the device's."""
    import torch
    S.til.set_validity(by_psi_half=vbp)
    pl, f = S.sheet(api), api.Fields(S.nx, S.ny, S.g, NCOMP, data=S.slab)
    S.til.fallback.zero_()
    api.AdvancePlasmaParticles(pl, f, S.geom, -1.0, 1.0, order, *PUSH, temp_slice=temp, n_subcycles=nsub, tiling=S.til)
    torch.cuda.synchronize()
    r2, v2 = S.real.copy(), S.valid.copy()
    oracle.advance_plasma(S.slab, S.nx, S.ny, S.g, r2, v2, S.ion, S.ogeom, PUSH, -1.0, 1.0, order, temp, nsub)
    greal, gvalid = pl.numpy()
    assert np.array_equal(gvalid, v2)
    live = v2 != 0
    for k in range(11):
        if live.any():
            err = rel_err(greal[k][live], r2[k][live])
            assert err < 1e-10, (k, err)
    gone = gvalid == 0
    assert np.all(greal[2][gone] == 0.0) and np.all(greal[10][gone] == 0.0), "an invalid particle kept its weight or psi_half"
    was = S.valid == 0
    assert np.array_equal(greal[:, was], S.real[:, was]), "a record that was invalid before the push was written"
    assert np.array_equal(f.numpy(), S.slab)
    assert S.til.fallback.item() == expect_fallback
    return r2, v2, greal


def _variants(order, ts):
    """(valid-by-weight deposition, valid-by-psi_half push): the engine's variants exist at order 2 on 16 x 16 tiles."""
    return [(False, False), (True, True)] if (order, ts) == (2, 16) else [(False, False), (True, False)]


POP_CASES = [(2, 16, (48, 32)), (2, 32, (48, 32)), (0, 16, (48, 32)), (3, 32, (48, 32)),
             (2, 16, (17, 9)), (2, 32, (17, 9)), (3, 16, (17, 9)), (0, 32, (17, 9))]


@pytest.mark.parametrize("case", POP_CASES, ids=lambda c: f"o{c[0]}-t{c[1]}-{c[2][0]}x{c[2][1]}")
def test_tile_populations(api, oracle, case):
    order, ts, (nx, ny) = case
    nt = ((nx + ts - 1) // ts) * ((ny + ts - 1) // ts)
    for k, start in enumerate(range(0, len(POPS), nt)):
        pops = [POPS[(start + t) % len(POPS)] for t in range(nt)]
        S = Sheet(api, oracle, nx, ny, ts, order, pops, 900 + 10 * order + k)
        # a few invalid records anywhere, so that the validity variants have something to skip
        S.invalidate(np.arange(3, S.n, 23))
        for vbw, vbp in _variants(order, ts):
            _explicit(api, oracle, S, order, vbw, 0)
            _push(api, oracle, S, order, vbp)


def _boundary_positions(pop, which):
    """Positions 256 k + d (d in `which`) that exist in a tile of `pop` records."""
    return sorted({256 * k + d for k in range(0, pop // 256 + 2) for d in which if 0 <= 256 * k + d < pop})


@pytest.mark.parametrize("order,ts", [(2, 16), (2, 32), (0, 16), (3, 32)])
def test_invalid_records_on_thread_boundaries(api, oracle, order, ts):
    nx, ny = 48, 32
    S = Sheet(api, oracle, nx, ny, ts, order, [769, 770, 513, 1025, 300, 768] if ts == 16 else [1025, 769], 40 + order + ts)
    nt = S.pops.size
    which = [(-1, 0, 1), (-1,), (0,), (1,), None, (-1, 1)]
    for t in range(nt):
        w = which[t % len(which)]
        if w is None:
            S.invalidate(S.first[t] + np.arange(S.pops[t]))      # a tile without a valid record
        else:
            S.invalidate([S.record(t, p) for p in _boundary_positions(S.pops[t], w)])
    for vbw, vbp in _variants(order, ts):
        _explicit(api, oracle, S, order, vbw, 0)
        _push(api, oracle, S, order, vbp)
    # every record invalid: nothing is deposited, nothing is pushed
    S.invalidate(np.arange(S.n))
    for vbw, vbp in _variants(order, ts):
        _explicit(api, oracle, S, order, vbw, 0)
        _push(api, oracle, S, order, vbp)


@pytest.mark.parametrize("temp", [0, 1])
@pytest.mark.parametrize("nsub", [1, 2, 3])
def test_push_subcycles_with_absorbing_boundary(api, oracle, nsub, temp):
    """Particles that fly at the x = hi wall from 0 to 1.2 steps of their own away from it: absorbed in the first or in a
    later sub-cycle (a sub-cycle advances by dz / n_subcycles), or not at all.  One absorbed in a later sub-cycle keeps the
    position the sub-cycle before has committed; one absorbed in the first keeps the position it came with."""
    nx, ny, dz = 48, 32, 0.3
    for order, ts, vbp in [(2, 16, False), (2, 16, True), (3, 32, False)]:
        S = Sheet(api, oracle, nx, ny, ts, order, [769, 513, 257, 512, 255, 770] if ts == 16 else [1025, 769], 70 + nsub + order,
                  bc=2, dz=dz)
        # the tiles along x = hi: records on the boundaries of the threads' sequences and in between
        flyers = []
        for t in range(S.pops.size):
            if t % S.ntx == S.ntx - 1:
                flyers += [S.record(t, p) for p in range(0, S.pops[t], 7)]
                flyers += [S.record(t, p) for p in _boundary_positions(S.pops[t], (-1, 0, 1))]
        fl = np.array(sorted(set(flyers)))
        step = dz * 1.0 / np.sqrt(2.0)                 # ux = 1, uy = uz = 0: psi = sqrt(2), ux / psi
        dist = step * 1.2 * (np.arange(fl.size) + 0.5) / fl.size
        S.real[0, fl] = HI[0] - dist
        S.real[6, fl] = S.real[0, fl]
        S.real[3, fl], S.real[4, fl], S.real[5, fl] = 1.0, 0.0, np.sqrt(2.0)
        S.real[8, fl], S.real[9, fl], S.real[10, fl] = 1.0, 0.0, np.sqrt(2.0)
        S.invalidate(np.arange(5, S.n, 31))
        before = S.valid.copy()
        r2, v2, greal = _push(api, oracle, S, order, vbp, nsub=nsub, temp=temp)
        absorbed = (before != 0) & (v2 == 0)
        first = absorbed & (r2[0] == S.real[0])
        later = absorbed & (r2[0] != S.real[0])
        assert first.sum() > 3, "no particle was absorbed in the first sub-cycle"
        if nsub > 1 and not temp:
            assert later.sum() > 3, "no particle was absorbed in a later sub-cycle"
        else:
            assert later.sum() == 0
        # what an absorbed particle leaves behind: the positions as the oracle leaves them, exactly unchanged if it left at once
        assert np.array_equal(greal[0][first], S.real[0][first]) and np.array_equal(greal[1][first], S.real[1][first])
        if later.any():
            assert rel_err(greal[0][later], r2[0][later]) < 1e-10 and rel_err(greal[1][later], r2[1][later]) < 1e-10
        # the record behind an absorbed one (the next of the sheet and the next of the same thread) is pushed as ever:
        # _push has compared every live record with the oracle; here: such records exist
        idx = np.nonzero(absorbed)[0]
        assert np.any(v2[np.minimum(idx + 1, S.n - 1)] != 0) and np.any(v2[np.minimum(idx + 256, S.n - 1)] != 0)


@pytest.mark.parametrize("order,ts", [(2, 16), (2, 32), (3, 16), (0, 32)])
def test_stale_sort(api, oracle, order, ts):
    nx, ny = 48, 32
    pops = [769, 1025, 513, 770, 1024, 300] if ts == 16 else [1025, 1300]
    # one per workgroup
    S = Sheet(api, oracle, nx, ny, ts, order, pops, 11 + order + ts)
    for t in range(S.pops.size):
        S.move_far(t, [S.record(t, (97 * (t + 1)) % S.pops[t])])
    S.invalidate(np.arange(9, S.n, 41))
    moved = int(S.pops.size - sum(S.valid[S.record(t, (97 * (t + 1)) % S.pops[t])] == 0 for t in range(S.pops.size)))
    for vbw, vbp in _variants(order, ts):
        _explicit(api, oracle, S, order, vbw, moved)
        _push(api, oracle, S, order, vbp, expect_fallback=moved)
    # several consecutive records of one thread: the first thread, one in the middle, the last thread with a record
    # in every round, and the thread that holds the tile's last record.  (dz = 0.05: no particle travels a cell per push, so
    # with sub-cycles the moved particles stay the only ones outside their tile's image and the counter stays predictable.)
    S = Sheet(api, oracle, nx, ny, ts, order, pops, 12 + order + ts, dz=0.05)
    far = []
    for t in range(S.pops.size):
        p = int(S.pops[t])
        rounds = (p - 1) // 256 + 1
        lanes = {0: range(rounds), 100: range(min(rounds, 3)), 255: range(p // 256), (p - 1) % 256: range(max(rounds - 2, 0), rounds)}
        idx = sorted({S.record(t, lane + 256 * m) for lane, ms in lanes.items() for m in ms if lane + 256 * m < p})
        if t % 2 == 0 or S.pops.size == 2:
            S.move_far(t, idx)
            far += idx
    far = np.array(far)
    assert far.size >= 8
    for vbw, vbp in _variants(order, ts):
        _explicit(api, oracle, S, order, vbw, far.size)
        _push(api, oracle, S, order, vbp, expect_fallback=far.size)
    # with sub-cycles every sub-cycle of a moved particle takes the slab path
    _push(api, oracle, S, order, False, nsub=2, temp=0, expect_fallback=2 * far.size)
    _push(api, oracle, S, order, False, nsub=3, temp=1, expect_fallback=3 * far.size)


def test_tail_workgroups_of_an_ionising_engine(api, oracle):
    """The electrons an ionisable species releases are appended behind the tile-sorted body of their sheet and worked on by
    tail workgroups of the three tile kernels until the next sort (256 records each, no tile image): one step of the
    ionisation deck against the oracle's engine."""
    deck = decks.ionization_SI()
    deck.update(n_steps=1)
    ge = api.SliceEngine(deck, tile_size=16)
    ge.set_diagnostics(True)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    for k in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(k)
        oe.solve_slice(k)
    gs, os_ = ge.slab(), oe.slab()
    for c, name in enumerate(ge.comp_names()):
        scale = max(np.abs(os_[c]).max(), 1e-300)
        assert np.abs(gs[c] - os_[c]).max() <= 1e-8 * scale, (name, np.abs(gs[c] - os_[c]).max() / scale)
    n_ion, n_el = ge.ion_stats()
    er, ev = ge.particles()
    orl, ovl = oe.particles()
    assert n_el == orl.shape[1] and n_el > 0, "the step released no electron: no tail workgroup ran"
    assert n_ion == oe.n_ionized()
    assert er.shape == orl.shape and np.array_equal(np.sort(ev), np.sort(ovl))
