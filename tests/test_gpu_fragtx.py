"""GPU: IPv4 TX fragmentation (pico_ipv4_fragment_batch_dev) against the numpy restatement of its
contract (tests/fragtx_ref.py, pinned to the compiled reference stack's own fragments by
tests/test_ref_fragtx.py) and against those fragments themselves (tests/golden/ref_fragtx_cases.npz).
Every comparison is over the WHOLE output buffer, pre-filled with a canary: a byte the contract does
not write -- outside a region, between two fragments, anywhere in a MALFORMED datagram's region --
must keep it."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests import fragtx_ref as R
from tests import test_ref_fragtx as RF
from tests.gpu_util import DEV, pairs_dev as grp_dev, replay_captured, to_dev

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def gpu_fragment(base, dd, mtu, groups, n_frag, out_size, od, stride, flags=0):
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * max(n_frag, 1), dtype=torch.uint8, device=DEV)
    v, c, l4 = batch.ipv4_fragment_batch(to_dev(base), to_dev(dd.view(np.uint8)), mtu, grp_dev(groups), n_frag, out,
                                         to_dev(od.view(np.uint8)), stride, flags=flags, out_frag=of)
    torch.cuda.synchronize()
    return (v.cpu().numpy(), c.cpu().numpy().view(np.uint32), l4.cpu().numpy().view(np.uint16),
            of.cpu().numpy().view(R.DESC_DTYPE)[:n_frag], out.cpu().numpy())


def check(base, dd, mtu, groups, n_frag, out_size, od, stride, flags=0):
    """GPU == restatement on every output and on every byte of the output buffer."""
    want_out = np.full(out_size, CANARY, np.uint8)
    wv, wc, w4, wof = R.fragment(base, dd, mtu, groups, n_frag, want_out, od, stride, flags)
    gv, gc, g4, gof, got_out = gpu_fragment(base, dd, mtu, groups, n_frag, out_size, od, stride, flags)
    np.testing.assert_array_equal(gv, wv)
    np.testing.assert_array_equal(gc, wc)
    np.testing.assert_array_equal(g4, w4)
    np.testing.assert_array_equal(gof, wof)
    bad = np.flatnonzero(got_out != want_out)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8].tolist()}"
    return wv, wc, w4, wof, got_out


def synth_case(lengths, mtu, stride, seed, proto=17, align=0, out_off=12, spare=0):
    buf, off, dlen, groups, ooff, cap, n_frag, out_size = synth.ipv4_oversized(
        lengths, mtu=mtu, stride=stride, seed=seed, proto=proto, align=align, out_off=out_off, spare=spare)
    return buf, batch.make_desc(off, dlen), groups, n_frag, out_size, batch.make_desc(ooff, cap)


def test_reference_fixture():
    """MTU 1500, no flags: every fragment the compiled reference stack emitted, byte for byte."""
    dg = RF.datagrams(*RF.fixture()[:4])
    lens = np.array([d.size for d, _ in dg], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    base = np.concatenate([d for d, _ in dg])
    cnt = np.array([len(f) for _, f in dg], np.uint32)
    groups = np.stack([np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.uint32), cnt], axis=1)
    cap = cnt.astype(np.int64) * 1504
    ooff = 12 + np.concatenate([[0], np.cumsum(cap[:-1])])
    od = batch.make_desc(ooff, cap)
    wv, wc, w4, wof, out = check(base, batch.make_desc(offs, lens), 1500, groups, int(cnt.sum()), int(ooff[-1] + cap[-1] + 16),
                                 od, 1504)
    assert (wv == batch.V_ACCEPT).all()
    np.testing.assert_array_equal(wc, cnt)
    for g, (_, frs) in enumerate(dg):
        for k, f in enumerate(frs):
            d = wof[groups[g, 0] + k]
            assert int(d["len"]) == f.size
            np.testing.assert_array_equal(out[int(d["off"]):int(d["off"]) + f.size], f, err_msg=f"group {g} fragment {k}")


EDGE = [0, 1, 8, 1479, 1480, 1481, 2960, 2961, 65515]       # 65515: 45 fragments, len = 65535


@pytest.mark.parametrize("stride", [1500, 1504, 1536])
@pytest.mark.parametrize("out_off", [12, 1, 2, 3, 6, 11])
def test_edge_lengths_and_alignments(out_off, stride):
    """Every edge length at every source alignment 0..15, for output regions at out_off mod 16 and the
    three strides (1500: the source / destination shift changes from fragment to fragment)."""
    lengths = np.repeat(EDGE, 16)
    align = np.tile(np.arange(16), len(EDGE))
    proto = np.tile([17, 6, 1, 47], lengths.size // 4)
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, stride, 40, proto=proto, align=align, out_off=out_off)
    wv, wc, *_ = check(buf, dd, 1500, groups, n_frag, out_size, od, stride, flags=batch.F_WRITE if out_off & 1 else 0)
    assert (wv == batch.V_ACCEPT).all() and wc.max() == 45 and wc.min() == 1


@pytest.mark.parametrize("mtu,extra", [(28, 0), (28, 4), (68, 0), (576, 16), (1280, 0), (1280, 4), (1499, 8)])
def test_small_mtus(mtu, extra):
    """per = (mtu - 20) & ~7 for any MTU: 28 (per 8: 100 bytes in 13 fragments, the TCP crc in the
    third), 68, 576, 1280 (per 1256, which the reference misplaces), 1499 (a 1499-byte datagram goes
    out whole although its transport exceeds per)."""
    per = (mtu - 20) & ~7
    lengths = np.array([0, 1, 7, 8, 9, 17, 18, 100, per - 1, per, per + 1, 2 * per, 2 * per + 1, mtu - 20, mtu - 19, 3000])
    proto = np.tile([6, 17, 1, 200], 4)
    case = synth_case(lengths, mtu, 20 + per + extra, 41, proto=proto, align=np.arange(16) * 5 % 16, out_off=(mtu + extra) % 16)
    buf, dd, groups, n_frag, out_size, od = case
    for flags in (0, batch.F_WRITE):
        wv, wc, *_ = check(buf, dd, mtu, groups, n_frag, out_size, od, 20 + per + extra, flags)
        assert (wv == batch.V_ACCEPT).all()
        np.testing.assert_array_equal(wc, [synth.fragtx_count(int(x) + 20, mtu) for x in lengths])
    if mtu == 28:
        assert wc[7] == 13


def test_protocols_and_write():
    """TCP, UDP, ICMPv4 and an unknown protocol: d_out_transport against oracle.dualbuffer_checksum /
    oracle.checksum computed here from the datagram; F_WRITE changes the 2 crc bytes and nothing else."""
    lengths = np.array([20, 21, 1481, 4000, 9000, 2961] * 4)
    proto = np.repeat([6, 17, 1, 99], 6)
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 42, proto=proto, align=np.arange(24) % 16)
    _, _, l4, _, plain = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, 0)
    _, _, l4w, _, written = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    np.testing.assert_array_equal(l4, l4w)
    diff = np.zeros(out_size, bool)
    for g in range(lengths.size):
        o, ln, pr = int(dd["off"][g]), int(dd["len"][g]), int(proto[g])
        t = buf[o + 20:o + ln].copy()
        at = {6: 16, 17: 6, 1: 2}.get(pr)
        if at is None:
            assert l4[g] == 0
            continue
        t[at] = t[at + 1] = 0
        ph = np.concatenate([buf[o + 12:o + 20], np.array([0, pr, t.size >> 8, t.size & 0xFF], np.uint8)])
        want = O.checksum(t) if pr == 1 else O.dualbuffer_checksum(ph, t)
        assert l4[g] == want, (g, pr)
        p = int(od["off"][g]) + 20 + at
        assert (int(written[p]) << 8 | int(written[p + 1])) == want
        diff[p:p + 2] = True
    np.testing.assert_array_equal(plain[~diff], written[~diff])


def test_round_trip_on_the_device():
    """~300 datagrams of mixed lengths through ipv4_fragment_batch(F_WRITE), then
    ipv4_reassemble_batch on its output with the same groups: every datagram ACCEPT, its transport
    checksum verifying, its bytes the input's with the header normalised."""
    rng = np.random.default_rng(43)
    lengths = np.concatenate([rng.integers(8, 12000, 290), [65515, 1480, 1481, 2960, 20, 8, 44 * 1480, 30000, 9000, 1472]])
    n = lengths.size
    proto = np.where(np.arange(n) % 3 == 0, 6, 17)
    lengths = np.where((proto == 6) & (lengths < 20), 20, lengths)
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 44, proto=proto, align=rng.integers(0, 16, n))
    d_out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    d_of = torch.zeros(16 * n_frag, dtype=torch.uint8, device=DEV)
    d_grp = grp_dev(groups)
    v, c, l4 = batch.ipv4_fragment_batch(to_dev(buf), to_dev(dd.view(np.uint8)), 1500, d_grp, n_frag, d_out,
                                         to_dev(od.view(np.uint8)), 1504, flags=batch.F_WRITE, out_frag=d_of)
    cap = (lengths + 20).astype(np.int64)
    ro = 12 + np.concatenate([[0], np.cumsum((cap[:-1] + 31) // 16 * 16)])
    r_out = torch.zeros(int(ro[-1] + cap[-1] + 16), dtype=torch.uint8, device=DEV)
    ol, rl4, rv = batch.ipv4_reassemble_batch(d_out, d_of, n_frag, d_grp, r_out, to_dev(batch.make_desc(ro, cap).view(np.uint8)))
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == batch.V_ACCEPT).all() and (rv.cpu().numpy() == batch.V_ACCEPT).all()
    assert (rl4.cpu().numpy() == 0).all()
    np.testing.assert_array_equal(ol.cpu().numpy(), lengths)
    np.testing.assert_array_equal(c.cpu().numpy(), groups[:, 1])
    got, l4 = r_out.cpu().numpy(), l4.cpu().numpy().view(np.uint16)
    for g in range(n):
        o, ln = int(dd["off"][g]), int(dd["len"][g])
        want, have = buf[o:o + ln].copy(), got[int(ro[g]):int(ro[g]) + ln]
        want[[2, 3, 6, 7, 10, 11]] = have[[2, 3, 6, 7, 10, 11]]          # the first fragment's own len / frag / crc
        at = 36 if proto[g] == 6 else 26
        want[at], want[at + 1] = l4[g] >> 8, l4[g] & 0xFF
        np.testing.assert_array_equal(have, want, err_msg=f"datagram {g}")
        assert O.checksum(have[:20]) == 0


def test_malformed():
    """Every MALFORMED cause beside accepted neighbours: the verdicts, counts and slots of the
    restatement, and not one byte changed in a MALFORMED datagram's region or outside the regions."""
    lengths = np.full(12, 4000)
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 45, proto=17, align=np.arange(12), spare=1)
    dd, groups, od = dd.copy(), groups.copy(), od.copy()
    buf = buf[:int(dd["off"][11]) + 4020 - 1]          # 11: its region runs 1 byte past base_len
    dd["off"][1] = buf.size + 5                        # 1: starts past base_len
    dd["len"][2] = 19                                  # 2: len < 20
    dd["len"][3] = 65536                               # 3: len > 65535
    buf[int(dd["off"][4])] = 0x46                      # 4: IHL 6
    groups[5, 1] = 2                                   # 5: fewer reserved slots than its 3 fragments
    groups[6, 0] = n_frag - 2                          # 6: slots past n_frag
    od["len"][7] -= 1                                  # 7: region 1 byte too small
    od["off"][8] = out_size - 100                      # 8: region past out_len
    od["off"][9] = out_size + 1                        # 9: region starts past out_len
    wv, wc, w4, wof, out = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    np.testing.assert_array_equal(wv, [1, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, 8])
    np.testing.assert_array_equal(wc, [3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0])
    touched = np.zeros(out_size, bool)
    for g in (0, 10):
        for k in range(3):
            p = int(od["off"][g]) + 1504 * k
            touched[p:p + (1500 if k < 2 else 20 + 4000 - 2960)] = True
    assert (out[~touched] == CANARY).all()


def test_null_outputs_and_empty_batch():
    lengths = np.array([4000, 100, 9000])
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 46, proto=[6, 17, 1])
    wv, wc, w4, wof, want_out = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    args = (to_dev(buf), to_dev(dd.view(np.uint8)), 1500, grp_dev(groups), n_frag)
    d_od = to_dev(od.view(np.uint8))
    for skip in range(4):
        out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
        of = None if skip == 3 else torch.zeros(16 * n_frag, dtype=torch.uint8, device=DEV)
        res = [torch.full((3,), 77, dtype=dt, device=DEV) for dt in (torch.uint8, torch.int32, torch.int16)]
        if skip < 3:
            res[skip] = None
        v, c, l4 = batch.ipv4_fragment_batch(*args, out, d_od, 1504, flags=batch.F_WRITE, out_frag=of, results=tuple(res))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want_out)
        for t, w in ((v, wv), (c, wc), (l4, w4.view(np.int16))):
            if t is not None:
                np.testing.assert_array_equal(t.cpu().numpy(), w)
        if of is not None:
            np.testing.assert_array_equal(of.cpu().numpy().view(R.DESC_DTYPE), wof)
    # n_dgram == 0: nothing runs, nothing is written
    out = torch.full((64,), CANARY, dtype=torch.uint8, device=DEV)
    empty = torch.zeros(0, dtype=torch.int32, device=DEV)
    v, c, l4 = batch.ipv4_fragment_batch(args[0], torch.zeros(0, dtype=torch.uint8, device=DEV), 1500, empty, 0, out,
                                         torch.zeros(0, dtype=torch.uint8, device=DEV), 1504)
    torch.cuda.synchronize()
    assert v.numel() == 0 and (out.cpu().numpy() == CANARY).all()


def test_graph_replay():
    """One call captured into a graph and replayed twice: identical results each time."""
    lengths = np.array([4000, 65515, 100, 9000, 1481])
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1536, 47, proto=[6, 17, 1, 17, 6])
    wv, wc, w4, wof, want_out = check(buf, dd, 1500, groups, n_frag, out_size, od, 1536, batch.F_WRITE)
    args = (to_dev(buf), to_dev(dd.view(np.uint8)), 1500, grp_dev(groups), n_frag)
    d_od = to_dev(od.view(np.uint8))
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * n_frag, dtype=torch.uint8, device=DEV)
    res = batch.ipv4_fragment_batch(*args, out, d_od, 1536, flags=batch.F_WRITE, out_frag=of)      # warm (eager)
    torch.cuda.synchronize()

    def call(s):
        batch.ipv4_fragment_batch(*args, out, d_od, 1536, flags=batch.F_WRITE, out_frag=of, stream=s, results=res)

    def reset():
        out.fill_(CANARY)
        of.zero_()
        for r in res:
            r.zero_()

    def same():
        np.testing.assert_array_equal(out.cpu().numpy(), want_out)
        np.testing.assert_array_equal(of.cpu().numpy().view(R.DESC_DTYPE), wof)
        np.testing.assert_array_equal(res[0].cpu().numpy(), wv)
        np.testing.assert_array_equal(res[1].cpu().numpy().view(np.uint32), wc)
        np.testing.assert_array_equal(res[2].cpu().numpy().view(np.uint16), w4)

    replay_captured(call, reset, same)


def test_large_batch_one_wave_per_datagram():
    """Batches of 3072 datagrams or more run one wave per datagram (smaller ones four): 3200 mixed
    datagrams of 0 .. 4 fragments, every source alignment, F_WRITE."""
    rng = np.random.default_rng(48)
    n = 3200
    lengths = rng.integers(0, 4500, n)
    lengths[:8] = [0, 1, 1479, 1480, 1481, 2960, 2961, 4440]
    proto = np.array([6, 17, 1, 89])[rng.integers(0, 4, n)]
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 49, proto=proto, align=rng.integers(0, 16, n),
                                                       out_off=5)
    wv, wc, *_ = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    assert (wv == batch.V_ACCEPT).all() and wc.max() == 4
