"""The batches of tests/test_gpu_frag_regions.py (tests/frag_regions.py) through the oracle alone (CPU
only): what the GPU tests take for granted about them is known to hold before a GPU is involved -- the
unit grid is reassembled throughout, to the lengths its items state, and leaves no unspecified byte;
in the neighbour batch every datagram that is not reassembled stands between two reassembled ones in
tight regions; and the oracle itself leaves every pad and guard byte as the canary."""
from __future__ import annotations

import numpy as np
import pytest

from tests import frag_regions as R


def canary_left(case, out):
    """Every byte outside every region -- the pads between them and the guard -- is the canary."""
    inside = np.zeros(out.size, bool)
    for o, n in zip(case.od["off"].tolist(), case.od["len"].tolist()):
        inside[o:o + n] = True
    assert inside[:case.size].sum() < case.size or case.od.shape[0] < 2      # there are pads at all
    assert not inside[case.size:].any()
    R.same_bytes(out[~inside], np.full(int((~inside).sum()), R.CANARY, np.uint8), "pad and guard bytes")


def test_unspecified_mask():
    od = R.G.ipv4_desc(np.array([0, 40, 100, 150, 190], np.uint64), np.array([30, 50, 40, 30, 0], np.uint32))
    m = R.unspecified_mask(170, od, np.array([1, 8, 2, 8, 8]), np.array([10, 0, 15, 0, 0]), 20)
    want = np.zeros(170, bool)
    want[40:90] = True                                   # not reassembled: the region
    want[135:140] = True                                 # reassembled: past hdr + len
    want[150:170] = True                                 # clipped to the buffer
    np.testing.assert_array_equal(m, want)


def test_grid_items():
    assert len(R.ITEMS) == 384 + 2 * 2304 and len(R.ITEMS[::3]) == 1664
    al = {par + 2 * ((L + place // 4) % 8) for m, P, L, place, par in R.ITEMS}
    assert al == set(range(16))


@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("every", [1, 3])
def test_grid(v6, every):
    case = R.grid_case(v6, every)
    wl, w4, wv, out = R.oracle_of("grid", v6, every)
    assert (wv != R.MALFORMED).all() and set(wv.tolist()) == {1, 4}          # ACCEPT and L4_BAD
    np.testing.assert_array_equal(wl, [R.item_length(it) for it in R.ITEMS[::every]])
    np.testing.assert_array_equal(wl, case.length)
    assert case.tight.all() and (case.od["off"] % 4 == 0).all()
    assert R.unspecified_mask(out.size, case.od, wv, wl, R.hdr_of(v6)).sum() == 0
    place = (case.od["off"] + np.uint64(R.hdr_of(v6))) % np.uint64(16)
    np.testing.assert_array_equal(place, [it[3] for it in R.ITEMS[::every]])
    src = case.d["off"][case.grp[:, 0]] % np.uint64(16)                      # the first arrival's header
    np.testing.assert_array_equal(src, [it[4] + 2 * ((it[2] + it[3] // 4) % 8) for it in R.ITEMS[::every]])
    assert case.buf.size == int(case.d["off"][-1]) + int(case.d["len"][-1])
    canary_left(case, out)


@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("with_grid", [False, True])
def test_neighbours(v6, with_grid):
    case = R.neighbour_case(v6, with_grid)
    wl, w4, wv, out = R.oracle_of("neighbours", v6, with_grid)
    ok = wv != R.MALFORMED
    np.testing.assert_array_equal(np.where(ok, wl.astype(np.int64), -1), case.length)   # as constructed
    assert R.flanked(case, wv)
    assert ok.mean() >= 0.5
    assert (~ok).sum() == 15 and (case.grp[:, 1] > 128).sum() >= 3
    assert ((case.od["off"] % 4 == 0) | ~ok).all()
    canary_left(case, out)


@pytest.mark.parametrize("v6", [False, True])
def test_one_byte_less_of_capacity(v6):
    """A tight region is tight: one byte less and exactly that datagram is not reassembled."""
    case = R.grid_case(v6, 3)
    wl, w4, wv, out = R.oracle_of("grid", v6, 3)
    od = case.od.copy()
    pick = np.arange(5, od.shape[0], 97)
    od["len"][pick] -= 1
    _, _, v, _ = R.run_oracle(case, v6, od)
    np.testing.assert_array_equal(np.flatnonzero(v == R.MALFORMED), pick)
