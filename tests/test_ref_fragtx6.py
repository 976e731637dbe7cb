"""The IPv6 TX fragmentation contract pinned to the reference's receiver.

tests/golden/ref_fragtx6_cases.npz (tests/golden/make_ref_fragtx6.py): unfragmented IPv6 datagrams
and the fragments the restatement of pico_ipv6_fragment_batch_dev's contract (tests/fragtx6_ref.py)
cuts from them; when the fixture was made, the unmodified reference stack reassembled every
fragmented row (pico_ipv6_process_frag, modules/pico_fragments.c:432-498) into the datagram it was
cut from (column `pinned`; a datagram sent whole is no fragment: pinned by the restatement alone).
Here (no GPU): the restatement still reproduces the fixture, its fragments go through the oracle's
reassembly and its IPv6 check, and -- where oracle/_ref is built -- through the live reference."""
from __future__ import annotations

import os

import numpy as np
import pytest

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests import fragtx6_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MTUS = (1280, 1500, 72)
CANARY = 0xA5


def fixture(mtu):
    c = np.load(os.path.join(GOLDEN, "ref_fragtx6_cases.npz"))
    return {k[len(f"m{mtu}_"):]: c[k] for k in c.files if k.startswith(f"m{mtu}_")}


def run_ref(c, mtu, flags=R.F_WRITE):
    """The restatement on a fixture case; returns (out, out_frag, verdict, count, transport)."""
    out = np.full(int(c["out_size"][0]), CANARY, np.uint8)
    n_frag = c["slot_off"].size
    v, cnt, l4, of = R.fragment(c["buf"], batch.make_desc(c["off"], c["len"], c["id"]), mtu, c["groups"], n_frag, out,
                                batch.make_desc(c["out_off"], c["out_cap"]), int(c["stride"][0]), flags)
    return out, of, v, cnt, l4


def test_fixture_shape():
    rows = frs = 0
    for mtu in MTUS:
        c = fixture(mtu)
        T = c["len"].astype(np.int64) - 40
        per = (mtu - 48) & ~7
        assert set(c["proto"].tolist()) == {6, 17, 58}
        np.testing.assert_array_equal(c["count"], [synth.fragtx6_count(int(x), mtu) for x in c["len"]])
        np.testing.assert_array_equal(c["count"], np.where(T + 40 <= mtu, 1, -(-T // per)))
        np.testing.assert_array_equal(c["pinned"], c["count"] > 1)          # every fragmented row, no whole one
        assert {mtu - 40, mtu - 39, 2 * per - 1, 2 * per, 2 * per + 1} <= set(T.tolist()) and T.min() == 1
        assert c["slot_off"].size == c["count"].sum() == c["groups"][:, 1].sum()
        rows, frs = rows + T.size, frs + int(c["count"].sum())
    assert fixture(1500)["len"].max() == 6040 and fixture(1280)["count"].max() == 5
    assert (rows, frs) == (42, 121)


@pytest.mark.parametrize("mtu", MTUS)
def test_restatement_reproduces_the_fixture(mtu):
    c = fixture(mtu)
    out, of, v, cnt, l4 = run_ref(c, mtu)
    assert (v == R.V_ACCEPT).all()
    np.testing.assert_array_equal(out, c["exp_out"])
    np.testing.assert_array_equal(of["off"], c["slot_off"])
    np.testing.assert_array_equal(of["len"], c["slot_len"])
    assert (of["seed"] == 0).all()
    np.testing.assert_array_equal(cnt, c["count"])
    np.testing.assert_array_equal(l4, c["transport"])


@pytest.mark.parametrize("mtu", MTUS)
def test_transport_is_the_fused_batch_tx_value(mtu):
    """d_out_transport is what the fused IPv6 batch's TX rule gives for the datagram unfragmented
    (oracle.batch_ipv6 with tx; payload length = T): 0 where that batch computes none."""
    c = fixture(mtu)
    buf = c["buf"].copy()
    o, T = c["off"].astype(np.int64), c["len"].astype(np.int64) - 40
    buf[o + 4], buf[o + 5] = T >> 8, T & 0xFF
    l4, v = O.batch_ipv6(buf, batch.make_desc(c["off"], c["len"]), tx=True)
    np.testing.assert_array_equal(c["transport"], l4)
    short = T < np.array([R.MIN_HDR[int(p)] for p in c["proto"]])
    np.testing.assert_array_equal(v, np.where(short, R.V_MALFORMED, R.V_ACCEPT))
    assert (c["transport"][short] == 0).all() and short.any()


@pytest.mark.parametrize("mtu", MTUS)
def test_fragments_reassemble_to_the_transport(mtu):
    """The restatement's fragments (F_WRITE) through oracle.ipv6_reassemble, slots and groups as they
    are: the transport again, behind fragment 0's header, its checksum verifying (0)."""
    c = fixture(mtu)
    out, of, v, cnt, l4 = run_ref(c, mtu)
    rows = np.flatnonzero(cnt > 1)
    cap = c["len"][rows].astype(np.int64)
    ro = 8 + np.concatenate([[0], np.cumsum((cap[:-1] + 31) // 16 * 16)])      # (regions on 8 mod 16)
    rout = np.zeros(int(ro[-1] + cap[-1] + 16), np.uint8)
    ol, rl4, rv = O.ipv6_reassemble(out, of, c["groups"][rows], rout, batch.make_desc(ro, cap), nxthdr_dispatch=True)
    assert (rv == R.V_ACCEPT).all() and (rl4 == 0).all()
    for i, g in enumerate(rows):
        o, ln, pr = int(c["off"][g]), int(c["len"][g]), int(c["proto"][g])
        assert ol[i] == ln - 40
        want = c["buf"][o + 40:o + ln].copy()
        if ln - 40 >= R.MIN_HDR[pr]:
            want[R.CRC_AT[pr]], want[R.CRC_AT[pr] + 1] = l4[g] >> 8, l4[g] & 0xFF
        p = int(ro[i])
        np.testing.assert_array_equal(rout[p + 40:p + ln], want, err_msg=f"datagram {g}")
        f0 = int(of["off"][c["groups"][g, 0]])
        np.testing.assert_array_equal(rout[p:p + 40], out[f0:f0 + 40])          # fragment 0's header: nxthdr 44
        assert rout[p + 6] == 44


@pytest.mark.parametrize("mtu", MTUS)
def test_fragments_walk_to_frag_and_whole_datagrams_to_accept(mtu):
    """The oracle's IPv6 RX check on every emitted frame: a fragment is V_FRAG (handed to reassembly),
    a datagram sent whole ACCEPT with its written checksum verifying."""
    c = fixture(mtu)
    out, of, v, cnt, l4 = run_ref(c, mtu)
    whole = np.repeat(cnt == 1, cnt)
    proto = np.repeat(c["proto"], cnt)
    tl = of["len"].astype(np.int64) - 40
    ok = ~whole | (tl >= np.array([{6: 20, 17: 8, 58: 1}[int(p)] for p in proto]))   # (RX reads ahead to the field it needs)
    rl4, rv = O.batch_ipv6(out, of, nxthdr_dispatch=True)
    np.testing.assert_array_equal(rv[ok], np.where(whole, R.V_ACCEPT, batch.V_FRAG)[ok])
    assert (rl4[ok & whole & (tl >= 8)] == 0).all() and (ok & whole).sum() >= 3 and (~whole).sum() >= 10
    for k in np.flatnonzero(~whole):
        f = out[int(of["off"][k]):int(of["off"][k]) + int(of["len"][k])]
        kind, net_len, pr, om = O.ipv6_walk_frag(f)
        assert (kind, net_len, pr) == (O.WALK_FRAG, 48, int(proto[k]))
        assert (int(f[4]) << 8 | int(f[5])) == f.size - 40 and (om & 6) == 0


REF_RX = os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "libref_rx.so")


@pytest.mark.skipif(not os.path.exists(REF_RX), reason="oracle/_ref/libref_rx.so not built here")
def test_live_reference_reassembles_the_fragments():
    """The generator's pin again, against the reference compiled here: every fragmented row is
    delivered with the input's transport, and the fixture is what the generator writes today."""
    from tests.golden import make_ref_fragtx6 as M
    from tests.golden.make_ref_reasm import ref_lib
    arrays = M.build(ref_lib())
    c = np.load(os.path.join(GOLDEN, "ref_fragtx6_cases.npz"))
    assert set(arrays) == set(c.files)
    for k in c.files:
        np.testing.assert_array_equal(arrays[k], c[k], err_msg=k)
