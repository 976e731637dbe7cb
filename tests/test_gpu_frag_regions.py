"""GPU: the reassembly batches (pico_ipv4_reassemble_batch_dev, pico_ipv6_reassemble_batch_dev) held to
the last clause of their contract -- "no byte outside the region is written" -- and to the rest of
it exactly: output regions TIGHT (od.len = header + len) and back to back, the whole output buffer
pre-filled with a canary and compared with the oracle's, pads between the regions and 64 guard bytes
behind them included, at every byte but unspecified_mask (tests/frag_regions.py, where the batches are
built; tests/test_frag_regions_cases.py holds their conditions on the oracle alone).

  * the unit grid: members x payload bytes x place in the 16-byte line x source alignment, in every
    launch shape (flat grid, one wave and four waves a datagram); all reassembled, nothing masked;
  * the neighbours of what is not reassembled: each such datagram (incomplete, region too small or
    wrapping, a fragment behind the last, repeated offsets, overlap, truncated, over the length limit,
    bad groups and regions) between two reassembled ones, whose bytes are compared;
  * the ends of both buffers: regions at and past out_len, and fragments at both ends of base, with
    0x00 and then 0xFF around it."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from picotcp_amd import batch
from tests import frag_regions as R
from tests.gpu_util import DEV, pairs_dev, to_dev

pytestmark = pytest.mark.gpu


def gpu_run(case, v6, mode, base=None, out_len=None):
    """(out_len, out_transport, verdict, the output allocation WITH its guard) of the device: d_out a
    view of the first `out_len` (default: case.size) bytes of a canary-filled allocation of case.size +
    GUARD.  base: the device tensor to read the fragments from (default: an upload of case.buf)."""
    big = torch.full((case.size + R.GUARD,), R.CANARY, dtype=torch.uint8, device=DEV)
    out = big[:case.size if out_len is None else out_len]
    fn = batch.ipv6_reassemble_batch if v6 else batch.ipv4_reassemble_batch
    batch.set_reasm_flat(mode)
    try:
        ol, l4, v = fn(to_dev(case.buf) if base is None else base, to_dev(case.d.view(np.uint8)), case.d.size,
                       pairs_dev(case.grp), out, to_dev(case.od.view(np.uint8)))
        torch.cuda.synchronize()
    finally:
        batch.set_reasm_flat(0)
    return ol.cpu().numpy().view(np.uint32), l4.cpu().numpy().view(np.uint16), v.cpu().numpy(), big.cpu().numpy()


def same_results(got, want):
    for g, w, what in zip(got[:3], want[:3], ("out_len", "out_transport", "verdict")):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:8].tolist()}: {g[bad[:8]].tolist()} for {w[bad[:8]].tolist()}"


# every: ITEMS[::every].  4992 datagrams: the flat grid (mode 0), one wave a datagram (mode 2, >= 3072);
# 1664: four waves a datagram (mode 2), the flat grid forced (mode 1)
GRID_SHAPES = {"flat": (1, 0), "one_wave": (1, 2), "four_waves": (3, 2), "flat_forced": (3, 1)}


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("shape", GRID_SHAPES)
def test_unit_grid(shape, v6):
    every, mode = GRID_SHAPES[shape]
    case = R.grid_case(v6, every)
    want = R.oracle_of("grid", v6, every)
    got = gpu_run(case, v6, mode)
    hdr = R.hdr_of(v6)
    for ol, _, v, out in (want, got):                    # nothing drops out of the comparison
        assert (v != R.MALFORMED).all()
        np.testing.assert_array_equal(ol, case.length)
        assert R.unspecified_mask(out.size, case.od, v, ol, hdr).sum() == 0
    same_results(got, want)
    R.same_bytes(got[3], want[3])


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("how", ["flat_forced", "four_waves", "behind_the_grid_one_wave"])
def test_neighbours(how, v6):
    with_grid = how == "behind_the_grid_one_wave"
    case = R.neighbour_case(v6, with_grid)
    want = R.oracle_of("neighbours", v6, with_grid)
    wl, _, wv, w_out = want
    assert R.flanked(case, wv) and (wv != R.MALFORMED).mean() >= 0.5
    assert case.grp.shape[0] >= 3072 if with_grid else case.grp.shape[0] < 512
    got = gpu_run(case, v6, 1 if how == "flat_forced" else 2)
    same_results(got, want)
    R.same_outside(got[3], w_out, R.unspecified_mask(w_out.size, case.od, wv, wl, R.hdr_of(v6)))


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("mode", [1, 2])
def test_the_end_of_out(mode, v6):
    """Five tight regions and two values of out_len: the end of region 2 -- that region ends exactly
    on out_len, regions 3 and 4 start behind it -- and one byte short of the end of region 3: off +
    len = out_len + 1, and region 4 has off > out_len.  The two that do not fit are MALFORMED with
    out_len 0 and checksum 0 (the oracle knows no out_len: it is given od.len = 0 for them), and from
    out_len on every byte of the allocation stays the canary."""
    hdr = R.hdr_of(v6)
    dg = R.grid_dgrams([(2, 16, 13, 4, 1), (3, 8, 21, 12, 0), (2, 24, 48, 0, 1), (2, 8, 7, 8, 0), (1, 8, 33, 4, 1)], v6)
    case = R.build(dg, v6)
    od = case.od
    od_o = od.copy()
    od_o["len"][3:] = 0
    want = R.run_oracle(case, v6, od_o)
    assert (want[2][:3] != R.MALFORMED).all() and (want[2][3:] == R.MALFORMED).all()
    for out_len in (int(od["off"][2] + od["len"][2]), int(od["off"][3] + od["len"][3]) - 1):
        assert od["off"][2] + od["len"][2] <= out_len < od["off"][4] and od["off"][3] + od["len"][3] > out_len
        got = gpu_run(case, v6, mode, out_len=out_len)
        same_results(got, want)
        assert (got[0][3:] == 0).all() and (got[1][3:] == 0).all() and (got[2][3:] == R.MALFORMED).all()
        mask = R.unspecified_mask(out_len, od, want[2], want[0], hdr)                 # clipped to d_out
        mask = np.concatenate([mask, np.zeros(want[3].size - out_len, bool)])         # behind it: all specified
        R.same_outside(got[3], want[3], mask)
        R.same_bytes(got[3][out_len:], np.full(got[3].size - out_len, R.CANARY, np.uint8), "bytes behind out_len")


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("mode", [1, 2])
def test_both_ends_of_base(mode, v6):
    """d_base a view of a larger allocation: its first byte the first header byte of a fragment, its
    last byte the last payload byte of another, at all 16 alignments of that end, with 0x00 and then
    0xFF in front and behind: results and bytes are the oracle's both times."""
    items = [(3, 8, 1 + 3 * k, (4 * k) % 16, k & 1) for k in range(12)] + [(2, 40, 47, 4, 1), (1, 8, 29, 12, 0)]
    dg = R.grid_dgrams(items, v6)
    dg[0].aligns[0] = 0                                  # the buffer starts with a header
    case = R.build(dg, v6)
    n = case.buf.size
    assert int(case.d["off"].min()) == 0 and int((case.d["off"] + case.d["len"]).max()) == n
    want = R.run_oracle(case, v6)
    assert (want[2] != R.MALFORMED).all()
    hdr = R.hdr_of(v6)
    mask = R.unspecified_mask(want[3].size, case.od, want[2], want[0], hdr)
    assert mask.sum() == 0
    body = torch.from_numpy(case.buf.copy()).to(DEV)
    for a in range(16):
        front = 64 + (a - n) % 16                        # (front + n) % 16 == a: the allocation is 16-byte aligned
        for fill in (0x00, 0xFF):
            big = torch.full((front + n + 64,), fill, dtype=torch.uint8, device=DEV)
            assert big.data_ptr() % 16 == 0
            big[front:front + n] = body
            got = gpu_run(case, v6, mode, base=big[front:front + n])
            same_results(got, want)
            R.same_bytes(got[3], want[3], f"bytes (end at {a} mod 16, 0x{fill:02X} around)")
