"""The tile re-sort places the particles of a tile in closed form (sort.hip: k_tile_place) instead of sorting a second
time, and ranks the tiles for the launch order by counting (k_tile_launch_order) instead of sorting them.

CPU: the placement formula, restated in numpy, gives the permutation and the offsets of two stable argsorts.
GPU: perm and offsets of api.Tiling.reorder equal oracle.tile_sort bit for bit, and the launch order is a permutation of
the tiles with counts not increasing and ties in ascending tile index -- on both sides of the tile count at which the
launch order goes from the counting kernel to the rocPRIM sort (ORDER_COUNT_MAX = 8192 tiles in sort.hip)."""
import numpy as np
import pytest

from tests.util import thermal_sheet

LO, HI = (-8.0, -8.0), (8.0, 8.0)
RANK_CAP = 16
ORDER_COUNT_MAX = 8192          # sort.hip: more tiles than this and the launch order is sorted by rocPRIM
SHAPES = [(32, 32, 16), (48, 40, 16), (64, 64, 32)]      # four tiles; partial tiles on two edges; four cells per thread


def sheet_from_counts(nx, ny, counts, rng):
    """A sheet with counts[j, i] particles nearest to cell (i, j), in random particle order."""
    jj, ii = np.nonzero(counts)
    rep = counts[jj, ii]
    ci, cj = np.repeat(ii, rep), np.repeat(jj, rep)
    n = ci.size
    sh = rng.permutation(n)
    ci, cj = ci[sh], cj[sh]
    dx, dy = (HI[0] - LO[0]) / nx, (HI[1] - LO[1]) / ny
    real = np.zeros((11, n))
    real[0] = LO[0] + (ci + 0.5 + 0.8 * (rng.random(n) - 0.5)) * dx
    real[1] = LO[1] + (cj + 0.5 + 0.8 * (rng.random(n) - 0.5)) * dy
    real[2] = 0.5 + rng.random(n)
    real[3:] = rng.normal(0.0, 0.1, (8, n))
    real[6], real[7] = real[0], real[1]
    return real, np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.int32)


def clustered_sheet(nx, ny, ts, seed):
    """Cells of exactly 14, 15, 16, 17 and several hundred particles (in the first tile and in the last, which is a
    partial one where the grid is no multiple of the tile), a thin background, one tile without a particle, one tile
    whose particles are all invalid, and about 10 % invalid particles scattered over the rest (the last tile included)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 4, (ny, nx))
    special = [14, 15, 16, 17, 300, 499, 15, 16]
    for k, c in enumerate(special):
        counts[1 + k // 4, 2 + 3 * (k % 4)] = c                     # first tile
        counts[ny - 2 - k // 4, nx - 3 - 2 * (k % 4)] = c           # last tile
    counts[0:ts, ts:2 * ts] = 0                                     # tile 1: empty
    real, valid, ion = sheet_from_counts(nx, ny, counts, rng)
    ci = np.floor((real[0] - LO[0]) / (HI[0] - LO[0]) * nx).astype(int)
    cj = np.floor((real[1] - LO[1]) / (HI[1] - LO[1]) * ny).astype(int)
    ntx = (nx + ts - 1) // ts
    valid[(cj // ts) * ntx + ci // ts == ntx] = 0                   # first tile of the second tile row: all invalid
    exact = (ci < ts) & (cj >= 1) & (cj <= 2)                       # the first tile's special cells keep their counts
    valid[(rng.random(valid.size) < 0.1) & ~exact] = 0
    return real, valid, ion


def thermal(nx, ny, ts, seed):
    real, valid, ion = thermal_sheet(nx, ny, LO, HI, ppc=2, seed=seed, jitter=9.0)
    valid[3::11] = 0
    return real, valid, ion


SHEETS = {"thermal": thermal, "clustered": clustered_sheet}


# ---- numpy restatement (sort.hip: cell_key with the row-by-row cell numbering, k_tile_place) --------------------------
def cell_keys(real, valid, nx, ny, ts):
    dx, dy = (HI[0] - LO[0]) / nx, (HI[1] - LO[1]) / ny
    xoff, yoff = 0.5 * (LO[0] + HI[0] - dx * (nx - 1)), 0.5 * (LO[1] + HI[1] - dy * (ny - 1))
    ci = np.clip(np.floor((real[0] - xoff) * (1.0 / dx) + 0.5).astype(np.int64), 0, nx - 1)
    cj = np.clip(np.floor((real[1] - yoff) * (1.0 / dy) + 0.5).astype(np.int64), 0, ny - 1)
    ntx, nty = (nx + ts - 1) // ts, (ny + ts - 1) // ts
    key = ((cj // ts) * ntx + ci // ts) * ts * ts + (cj % ts) * ts + ci % ts
    return np.where(valid != 0, key, ntx * nty * ts * ts), ntx * nty


def two_sorts(key1, ntiles, ncell):
    n = key1.size
    ordr = np.argsort(key1, kind="stable")
    ks = key1[ordr]
    first = np.searchsorted(ks, np.arange(ntiles * ncell + 2))
    rank = np.minimum(np.arange(n) - first[ks], RANK_CAP - 1)
    tile, cit = ks // ncell, ks % ncell
    key2 = (tile * RANK_CAP + rank) * ncell + cit
    pos = np.argsort(key2, kind="stable")
    off = np.searchsorted(key2[pos] // (RANK_CAP * ncell), np.arange(ntiles + 2))
    off[ntiles + 1] = n
    return ordr[pos].astype(np.uint32), off.astype(np.int32)


def one_sort_and_placement(key1, ntiles, ncell):
    n, cap = key1.size, RANK_CAP - 1
    ordr = np.argsort(key1, kind="stable")
    ks = key1[ordr]
    first = np.searchsorted(ks, np.arange(ntiles * ncell + 2))
    cnt = np.diff(first)[:ntiles * ncell].reshape(ntiles, ncell)                  # n[c] of every tile
    more = cnt[:, None, :] > np.arange(cap)[None, :, None]                       # [tile, rank, cell]: n[c] > rank
    cells_before = np.cumsum(more, axis=2) - more                                 # #{c' < c : n[c'] > rank}
    n_rank = more.sum(axis=2)                                                     # N(rank)
    ranks_before = np.cumsum(n_rank, axis=1) - n_rank                             # sum_{q < rank} N(q)
    over = np.maximum(cnt - cap, 0)
    over_before = np.cumsum(over, axis=1) - over
    perm = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    p = np.arange(first[ntiles * ncell])                                          # the valid particles' sorted positions
    c = ks[p]
    t, cit, r = c // ncell, c % ncell, p - first[c]
    rr = np.minimum(r, cap - 1)
    low = ranks_before[t, rr] + cells_before[t, rr, cit]
    high = n_rank.sum(axis=1)[t] + over_before[t, cit] + (r - cap)
    perm[first[t * ncell] + np.where(r < cap, low, high)] = ordr[p]
    perm[first[ntiles * ncell]:] = ordr[first[ntiles * ncell]:]                   # invalid: the order of the sort
    off = np.append(first[np.arange(ntiles + 1) * ncell], n)
    return perm, off.astype(np.int32)


@pytest.mark.parametrize("nx,ny,ts", SHAPES)
@pytest.mark.parametrize("kind", list(SHEETS))
def test_placement_formula_is_the_second_stable_sort(nx, ny, ts, kind):
    real, valid, _ = SHEETS[kind](nx, ny, ts, 7 + nx + ts)
    key1, ntiles = cell_keys(real, valid, nx, ny, ts)
    if kind == "clustered":
        cnt = np.bincount(key1, minlength=ntiles * ts * ts + 1)[:ntiles * ts * ts]
        assert {14, 15, 16, 17} <= set(cnt.tolist()) and cnt.max() >= 300          # the cap from both sides
        per_tile = cnt.reshape(ntiles, -1).sum(axis=1)
        assert (per_tile == 0).sum() >= 2                                          # the empty and the all-invalid tile
    perm2, off2 = two_sorts(key1, ntiles, ts * ts)
    perm1, off1 = one_sort_and_placement(key1, ntiles, ts * ts)
    assert np.array_equal(perm1, perm2)
    assert np.array_equal(off1, off2)


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def check_launch_order(til, off, ntiles):
    order, rec = til.launch_order()
    assert np.array_equal(np.sort(order), np.arange(ntiles))                       # a permutation of the tiles
    cnt = np.diff(off)[:ntiles][order]
    assert np.all(cnt[:-1] >= cnt[1:])                                             # heaviest first
    tie = cnt[:-1] == cnt[1:]
    assert np.all(order[:-1][tie] < order[1:][tie])                                # ties: ascending tile index
    assert np.array_equal(rec[:, 0], order)
    assert np.array_equal(rec[:, 1], off[order]) and np.array_equal(rec[:, 2], off[order + 1])
    assert not rec[:, 3].any()


def sort_both(api, oracle, real, valid, ion, nx, ny, ts):
    n = real.shape[1]
    til = api.Tiling(nx, ny, ts, n)
    out = til.reorder(api.PlasmaSheet(real, valid, ion), api.Geometry(nx, ny, LO, HI, 0.12))
    off, perm = til.offsets_and_perm(n)
    operm, ooff = oracle.tile_sort(real, valid, ion, oracle.make_geom(nx, ny, LO, HI, dz=0.12, bc=1), nx, ny, ts)
    assert np.array_equal(perm, operm)              # integer work: bit-exact
    assert np.array_equal(off, ooff)
    ntiles = off.size - 2
    check_launch_order(til, off, ntiles)
    return til, out, operm


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,ts", SHAPES)
@pytest.mark.parametrize("kind", list(SHEETS))
def test_gpu_placement_bit_exact(api, oracle, nx, ny, ts, kind):
    real, valid, ion = SHEETS[kind](nx, ny, ts, 7 + nx + ts)
    til, out, operm = sort_both(api, oracle, real, valid, ion, nx, ny, ts)
    greal, gvalid = out.numpy()
    assert np.array_equal(greal, real[:, operm])    # pure data movement: bit-exact
    assert np.array_equal(gvalid, valid[operm])
    # the same tiling again, with another sheet: nothing is left over from the sort before
    half = real.shape[1] // 2
    real, valid, ion = np.ascontiguousarray(real[:, ::-1][:, :half]), valid[::-1][:half].copy(), ion[:half].copy()
    til.reorder(api.PlasmaSheet(real, valid, ion), api.Geometry(nx, ny, LO, HI, 0.12))
    off, perm = til.offsets_and_perm(half)
    operm, ooff = oracle.tile_sort(real, valid, ion, oracle.make_geom(nx, ny, LO, HI, dz=0.12, bc=1), nx, ny, ts)
    assert np.array_equal(perm, operm) and np.array_equal(off, ooff)
    check_launch_order(til, off, off.size - 2)


@pytest.mark.gpu
@pytest.mark.parametrize("ts", [16, 32])
@pytest.mark.parametrize("n", [0, 1])
def test_gpu_placement_of_no_and_of_one_particle(api, oracle, ts, n):
    real, valid, ion = thermal_sheet(48, 40, LO, HI, ppc=1, seed=3, jitter=1.0)
    real, valid, ion = np.ascontiguousarray(real[:, 77:77 + n]), valid[77:77 + n].copy(), ion[77:77 + n].copy()
    sort_both(api, oracle, real, valid, ion, 48, 40, ts)


@pytest.mark.gpu
@pytest.mark.parametrize("ntx,nty", [(90, 91), (91, 91)])
def test_gpu_launch_order_on_both_sides_of_the_switch(api, oracle, ntx, nty):
    """8190 tiles: ranked by counting; 8281 tiles: sorted by rocPRIM.  A sparse sheet, so that the counts tie often, with
    a few heavy cells."""
    ts = 16
    assert (ntx * nty <= ORDER_COUNT_MAX) == (ntx == 90)
    nx, ny = ntx * ts - 5, nty * ts - 9
    rng = np.random.default_rng(ntx)
    counts = (rng.random((ny, nx)) < 0.01).astype(np.int64)
    counts[rng.integers(0, ny, 40), rng.integers(0, nx, 40)] = rng.integers(2, 40, 40)
    real, valid, ion = sheet_from_counts(nx, ny, counts, rng)
    valid[rng.random(valid.size) < 0.1] = 0
    sort_both(api, oracle, real, valid, ion, nx, ny, ts)
