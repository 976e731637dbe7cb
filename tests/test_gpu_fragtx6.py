"""GPU: IPv6 TX fragmentation (pico_ipv6_fragment_batch_dev) against the numpy restatement of its
contract (tests/fragtx6_ref.py, pinned to the compiled reference stack's reassembly by
tests/golden/make_ref_fragtx6.py and tests/test_ref_fragtx6.py) and against that fixture itself.
Every comparison is over the WHOLE output buffer, pre-filled with a canary: a byte the contract does
not write -- outside a region, between two fragments, anywhere in a MALFORMED datagram's region --
must keep it."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from picotcp_amd import batch, synth
from tests import fragtx6_ref as R
from tests import test_ref_fragtx6 as RF
from tests.gpu_util import DEV, pairs_dev as grp_dev, replay_captured, to_dev

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def gpu_fragment(base, dd, mtu, groups, n_frag, out_size, od, stride, flags=0):
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * max(n_frag, 1), dtype=torch.uint8, device=DEV)
    v, c, l4 = batch.ipv6_fragment_batch(to_dev(base), to_dev(dd.view(np.uint8)), mtu, grp_dev(groups), n_frag, out,
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


def synth_case(lengths, mtu, stride, seed, proto=17, align=0, out_off=0, spare=0):
    buf, off, dlen, ids, groups, ooff, cap, n_frag, out_size = synth.ipv6_oversized(
        lengths, mtu=mtu, stride=stride, seed=seed, proto=proto, align=align, out_off=out_off, spare=spare)
    return buf, batch.make_desc(off, dlen, ids), groups, n_frag, out_size, batch.make_desc(ooff, cap)


def up(x, m):
    return -(-x // m) * m


@pytest.mark.parametrize("mtu", RF.MTUS)
def test_reference_fixture(mtu):
    """The fixture's datagrams: the output buffer whose fragments the compiled reference reassembled."""
    c = RF.fixture(mtu)
    n_frag = c["slot_off"].size
    gv, gc, g4, gof, out = gpu_fragment(c["buf"], batch.make_desc(c["off"], c["len"], c["id"]), mtu, c["groups"], n_frag,
                                        int(c["out_size"][0]), batch.make_desc(c["out_off"], c["out_cap"]),
                                        int(c["stride"][0]), batch.F_WRITE)
    assert (gv == batch.V_ACCEPT).all()
    np.testing.assert_array_equal(gc, c["count"])
    np.testing.assert_array_equal(g4, c["transport"])
    np.testing.assert_array_equal(gof["off"], c["slot_off"])
    np.testing.assert_array_equal(gof["len"], c["slot_len"])
    assert (gof["seed"] == 0).all()
    np.testing.assert_array_equal(out, c["exp_out"])


SMALL_T = [1, 7, 8, 9, 16, 17, 18, 25]


@pytest.mark.parametrize("stride", [56, 64])
def test_mtu_56(stride):
    """per = 8: T up to 16 goes out whole, 17 / 18 / 25 in 3 / 3 / 4 fragments; a TCP crc field (T = 25)
    lies in fragment 2, UDP's and ICMPv6's in fragment 0; a transport shorter than its header gets no
    checksum.  Every source alignment, both flags."""
    lengths = np.repeat(SMALL_T, 6)
    proto = np.tile([6, 17, 58, 6, 17, 58], len(SMALL_T))
    case = synth_case(lengths, 56, stride, 80, proto=proto, align=np.arange(lengths.size) % 16, out_off=stride % 16 + 1)
    buf, dd, groups, n_frag, out_size, od = case
    for flags in (0, batch.F_WRITE):
        wv, wc, w4, wof, out = check(buf, dd, 56, groups, n_frag, out_size, od, stride, flags)
        assert (wv == batch.V_ACCEPT).all()
        np.testing.assert_array_equal(wc, np.repeat([1, 1, 1, 1, 1, 3, 3, 4], 6))
    g = int(np.flatnonzero((lengths == 25) & (proto == 6))[0])
    assert w4[g] != 0
    p = int(od["off"][g]) + 2 * stride + 48                        # fragment 2 carries transport bytes 16..23
    assert (int(out[p]) << 8 | int(out[p + 1])) == w4[g]
    assert (w4[(lengths < 20) & (proto == 6)] == 0).all() and (w4[(lengths >= 8) & (proto == 17)] != 0).all()


@pytest.mark.parametrize("out_off", [0, 1, 2, 3, 8, 15])
@pytest.mark.parametrize("mtu", [1280, 1499, 1500, 1501])
def test_edge_lengths_and_alignments(mtu, out_off):
    """T around every multiple of per (odd counts, a lone last fragment) at every source alignment 0..15,
    for output regions at out_off mod 16 and the strides 48 + per rounded up to 4 and to 16."""
    per = (mtu - 48) & ~7
    edge = [per - 1, per, per + 1, 2 * per, 2 * per + 1, 3 * per]
    lengths = np.repeat(edge, 16)
    align = np.tile(np.arange(16), len(edge))
    proto = np.tile([17, 6, 58, 47], lengths.size // 4)
    for stride in (up(48 + per, 4), up(48 + per, 16)):
        buf, dd, groups, n_frag, out_size, od = synth_case(lengths, mtu, stride, 81, proto=proto, align=align, out_off=out_off)
        wv, wc, *_ = check(buf, dd, mtu, groups, n_frag, out_size, od, stride, flags=batch.F_WRITE if out_off & 1 else 0)
        assert (wv == batch.V_ACCEPT).all()
        np.testing.assert_array_equal(wc, np.repeat([1, 1, 1, 2, 3, 3], 16))


def test_longest_datagram_and_the_buffers_last_byte():
    """len = 65535 (46 fragments at MTU 1500), and a datagram that ends at the last byte of d_base at
    every alignment of that end (the mover's last unit is read byte by byte)."""
    buf, dd, groups, n_frag, out_size, od = synth_case([65495], 1500, 1504, 82, proto=17, align=5, out_off=8)
    wv, wc, *_ = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    assert wv[0] == batch.V_ACCEPT and wc[0] == 46 and dd["len"][0] == 65535
    for a in range(16):
        buf, dd, groups, n_frag, out_size, od = synth_case([100, 3001], 1280, 1280, 83 + a, proto=[58, 6], align=[0, a])
        buf = buf[:int(dd["off"][1]) + int(dd["len"][1])]
        wv, wc, *_ = check(buf, dd, 1280, groups, n_frag, out_size, od, 1280, batch.F_WRITE)
        assert (wv == batch.V_ACCEPT).all() and wc.tolist() == [1, 3]


def test_protocols_and_write():
    """TCP, UDP, ICMPv6 and an unknown protocol: d_out_transport is what ipv6_checksum_batch(F_TX) reports
    for the datagram unfragmented, measured on the device here; F_WRITE changes the 2 crc bytes and
    nothing else; without it the transport is copied verbatim."""
    lengths = np.array([3, 20, 21, 1500, 4000, 9000, 2897] * 4)
    proto = np.repeat([6, 17, 58, 253], 7)
    n = lengths.size
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 84, proto=proto, align=np.arange(n) % 16)
    o = dd["off"].astype(np.int64)
    buf[o + 4], buf[o + 5] = lengths >> 8, lengths & 0xFF          # (the checksum batch reads the payload length)
    _, wc, l4, wof, plain = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, 0)
    _, _, l4w, _, written = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    np.testing.assert_array_equal(l4, l4w)
    tx4, txv = batch.ipv6_checksum_batch(to_dev(buf), to_dev(batch.make_desc(dd["off"], dd["len"]).view(np.uint8)), n,
                                         flags=batch.F_TX)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(l4, tx4.cpu().numpy().view(np.uint16))
    short = lengths < np.array([R.MIN_HDR.get(int(p), 0) for p in proto])
    np.testing.assert_array_equal(txv.cpu().numpy(), np.where(short, batch.V_MALFORMED, batch.V_ACCEPT))
    assert (l4[short | (proto == 253)] == 0).all() and (l4[~short & (proto != 253)] != 0).all()
    diff = np.zeros(out_size, bool)
    for g in range(n):
        hb = 40 if wc[g] == 1 else 48
        f0 = int(od["off"][g])
        np.testing.assert_array_equal(plain[f0 + hb:f0 + hb + min(int(lengths[g]), 1448)],
                                      buf[o[g] + 40:o[g] + 40 + min(int(lengths[g]), 1448)])     # verbatim
        at = R.CRC_AT.get(int(proto[g]))
        if at is None or short[g]:
            continue
        p = f0 + hb + at
        assert (int(written[p]) << 8 | int(written[p + 1])) == l4[g]
        diff[p:p + 2] = True
    np.testing.assert_array_equal(plain[~diff], written[~diff])


def roundtrip(d_base, d_dd, dgram_len, n, groups, n_frag, out_size, d_od, mtu, stride):
    """ipv6_fragment_batch(F_WRITE) then ipv6_reassemble_batch on its outputs as they are.  Returns the
    fragmentation's (out, out_frag, transport) and the reassembly's (regions, buffer) as host arrays."""
    d_out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    d_of = torch.zeros(16 * n_frag, dtype=torch.uint8, device=DEV)
    d_grp = grp_dev(groups)
    v, c, l4 = batch.ipv6_fragment_batch(d_base, d_dd, mtu, d_grp, n_frag, d_out, d_od, stride, flags=batch.F_WRITE,
                                         out_frag=d_of)
    cap = np.asarray(dgram_len, np.int64)
    ro = 8 + np.concatenate([[0], np.cumsum((cap[:-1] + 31) // 16 * 16)])
    r_out = torch.zeros(int(ro[-1] + cap[-1] + 16), dtype=torch.uint8, device=DEV)
    ol, rl4, rv = batch.ipv6_reassemble_batch(d_out, d_of, n_frag, d_grp, r_out, to_dev(batch.make_desc(ro, cap).view(np.uint8)),
                                              flags=batch.F_NXTHDR_DISPATCH)
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == batch.V_ACCEPT).all() and (rv.cpu().numpy() == batch.V_ACCEPT).all()
    assert (rl4.cpu().numpy() == 0).all()
    np.testing.assert_array_equal(ol.cpu().numpy(), cap - 40)
    np.testing.assert_array_equal(c.cpu().numpy(), groups[:, 1])
    return (d_out.cpu().numpy(), d_of.cpu().numpy().view(R.DESC_DTYPE), l4.cpu().numpy().view(np.uint16)), (ro, r_out.cpu().numpy())


def test_round_trip_on_the_device():
    """~200 datagrams above the MTU through ipv6_fragment_batch(F_WRITE), then ipv6_reassemble_batch
    (F_NXTHDR_DISPATCH) on d_out, d_out_frag and d_groups as they are: every datagram ACCEPT, out_len = T,
    its checksum verifying, the transport the input's, the header fragment 0's."""
    rng = np.random.default_rng(85)
    lengths = np.concatenate([rng.integers(1461, 12000, 190), [65495, 1461, 2896, 2897, 44 * 1448, 30000, 9000]])
    n = lengths.size
    proto = np.array([6, 17, 58])[np.arange(n) % 3]
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 86, proto=proto, align=rng.integers(0, 16, n))
    (out, of, l4), (ro, got) = roundtrip(to_dev(buf), to_dev(dd.view(np.uint8)), dd["len"], n, groups, n_frag, out_size,
                                         to_dev(od.view(np.uint8)), 1500, 1504)
    for g in range(n):
        o, ln, at = int(dd["off"][g]), int(dd["len"][g]), R.CRC_AT[int(proto[g])]
        want = buf[o + 40:o + ln].copy()
        want[at], want[at + 1] = l4[g] >> 8, l4[g] & 0xFF
        p = int(ro[g])
        np.testing.assert_array_equal(got[p + 40:p + ln], want, err_msg=f"datagram {g}")
        f0 = int(of["off"][groups[g, 0]])
        np.testing.assert_array_equal(got[p:p + 40], out[f0:f0 + 40])
        assert got[p + 6] == 44 and (int(got[p + 4]) << 8 | int(got[p + 5])) == 8 + 1448


def test_chain_behind_the_icmp6_answers():
    """Echo answers above 1280 bytes, which icmp6_reply_batch writes whole (its contract knows no MTU), go
    through the new batch at MTU 1280 as they lie -- its out / out_ans are base / dgram_desc -- and the
    fragments reassemble to the answers."""
    rng = np.random.default_rng(87)
    Ts = [1241, 1300, 2464, 2465, 9000]
    reqs = [synth.icmp6_echo_request(rng, T, 7, k) for k, T in enumerate(Ts)]
    buf, off, ln, req, ooff, cap, osize = synth.icmp6_burst(reqs, 0)
    n = len(Ts)
    ans = torch.zeros(osize, dtype=torch.uint8, device=DEV)
    av, aoa = batch.icmp6_reply_batch(to_dev(buf), to_dev(batch.make_desc(off, ln).view(np.uint8)), n,
                                      to_dev(req.view(np.uint8)), ans, to_dev(batch.make_desc(ooff, cap).view(np.uint8)))
    torch.cuda.synchronize()
    assert (av.cpu().numpy() == batch.V_ACCEPT).all()
    a_desc = aoa.cpu().numpy().view(R.DESC_DTYPE)
    np.testing.assert_array_equal(a_desc["len"], [40 + T for T in Ts])
    cnt = np.array([synth.fragtx6_count(40 + T, 1280) for T in Ts], np.uint32)
    assert cnt.tolist() == [2, 2, 2, 3, 8]
    groups = np.stack([np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.uint32), cnt], axis=1)
    fcap = cnt.astype(np.int64) * 1280
    fo = np.concatenate([[0], np.cumsum(fcap[:-1])])
    host_ans = ans.cpu().numpy()
    # (the whole-buffer comparison against the restatement, then the device round trip)
    check(host_ans, a_desc, 1280, groups, int(cnt.sum()), int(fcap.sum()) + 16, batch.make_desc(fo, fcap), 1280, batch.F_WRITE)
    (out, of, l4), (ro, got) = roundtrip(ans, aoa, a_desc["len"], n, groups, int(cnt.sum()), int(fcap.sum()) + 16,
                                         to_dev(batch.make_desc(fo, fcap).view(np.uint8)), 1280, 1280)
    for g, T in enumerate(Ts):
        o, p = int(a_desc["off"][g]), int(ro[g])
        np.testing.assert_array_equal(got[p + 40:p + 40 + T], host_ans[o + 40:o + 40 + T])   # (the answer's crc was valid: rewritten the same)
        assert (int(host_ans[o + 42]) << 8 | int(host_ans[o + 43])) == l4[g]


EXT = (0, 43, 44, 50, 51, 60, 135)


def test_malformed():
    """Every MALFORMED cause beside accepted neighbours: the verdicts, counts and slots of the
    restatement, and not one byte changed in a MALFORMED datagram's region or outside the regions."""
    n = 13 + len(EXT)
    lengths = np.full(n, 4000)
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 88, proto=17, align=np.arange(n) % 16, spare=1)
    dd, groups, od = dd.copy(), groups.copy(), od.copy()
    buf = buf[:int(dd["off"][n - 1]) + 4040 - 1]       # n - 1: its datagram runs 1 byte past base_len
    dd["off"][1] = buf.size + 5                        # 1: starts past base_len
    dd["len"][2] = 39                                  # 2: len < 40
    dd["len"][3] = 65536                               # 3: len > 65535
    buf[int(dd["off"][4])] = 0x45                      # 4: version 4
    groups[5, 1] = 2                                   # 5: fewer reserved slots than its 3 fragments
    groups[6, 0] = n_frag - 2                          # 6: slots past n_frag
    od["len"][7] -= 1                                  # 7: region 1 byte too small
    od["off"][8] = out_size - 100                      # 8: region past out_len
    od["off"][9] = out_size + 1                        # 9: region starts past out_len
    buf[int(dd["off"][10])] = 0x70                     # 10: version 7
    for k, nx in enumerate(EXT):                       # 12 ..: an extension header's value in nxthdr
        buf[int(dd["off"][12 + k]) + 6] = nx
    wv, wc, w4, wof, out = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    good = [0, 11]
    np.testing.assert_array_equal(wv, [1 if g in good else 8 for g in range(n)])
    np.testing.assert_array_equal(wc, [3 if g in good else 0 for g in range(n)])
    touched = np.zeros(out_size, bool)
    for g in good:
        for k in range(3):
            p = int(od["off"][g]) + 1504 * k
            touched[p:p + (1496 if k < 2 else 48 + 4000 - 2896)] = True
    assert (out[~touched] == CANARY).all()
    # slots past n_frag: no slot written; the others' reserved slots are {0, 0, 0}
    assert (wof["len"][groups[5, 0]:groups[5, 0] + 2] == 0).all()


def test_null_outputs_and_empty_batch():
    lengths = np.array([4000, 100, 9000])
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 89, proto=[6, 17, 58])
    wv, wc, w4, wof, want_out = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    args = (to_dev(buf), to_dev(dd.view(np.uint8)), 1500, grp_dev(groups), n_frag)
    d_od = to_dev(od.view(np.uint8))
    for skip in range(4):
        out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
        of = None if skip == 3 else torch.zeros(16 * n_frag, dtype=torch.uint8, device=DEV)
        res = [torch.full((3,), 77, dtype=dt, device=DEV) for dt in (torch.uint8, torch.int32, torch.int16)]
        if skip < 3:
            res[skip] = None
        v, c, l4 = batch.ipv6_fragment_batch(*args, out, d_od, 1504, flags=batch.F_WRITE, out_frag=of, results=tuple(res))
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
    v, c, l4 = batch.ipv6_fragment_batch(args[0], torch.zeros(0, dtype=torch.uint8, device=DEV), 1500, empty, 0, out,
                                         torch.zeros(0, dtype=torch.uint8, device=DEV), 1504)
    torch.cuda.synchronize()
    assert v.numel() == 0 and (out.cpu().numpy() == CANARY).all()


def test_graph_replay():
    """One call captured into a graph and replayed twice: identical results each time."""
    lengths = np.array([4000, 65495, 100, 9000, 1461])
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1536, 90, proto=[6, 17, 58, 17, 6])
    wv, wc, w4, wof, want_out = check(buf, dd, 1500, groups, n_frag, out_size, od, 1536, batch.F_WRITE)
    args = (to_dev(buf), to_dev(dd.view(np.uint8)), 1500, grp_dev(groups), n_frag)
    d_od = to_dev(od.view(np.uint8))
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * n_frag, dtype=torch.uint8, device=DEV)
    res = batch.ipv6_fragment_batch(*args, out, d_od, 1536, flags=batch.F_WRITE, out_frag=of)      # warm (eager)
    torch.cuda.synchronize()

    def call(s):
        batch.ipv6_fragment_batch(*args, out, d_od, 1536, flags=batch.F_WRITE, out_frag=of, stream=s, results=res)

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


def test_one_wave_shape_equals_four_wave_shape():
    """Batches of 3072 datagrams or more with at most 16 slots a datagram on average run one wave per
    datagram.  3200 mixed datagrams of 1 .. 4 fragments, every source alignment, F_WRITE: the
    restatement's result -- and the same result with n_frag above 16 a datagram (spare slots nobody
    reserves), which takes the four-wave shape on the same inputs."""
    rng = np.random.default_rng(91)
    n = 3200
    lengths = rng.integers(0, 4500, n)
    lengths[:9] = [0, 1, 1447, 1448, 1449, 1460, 1461, 2896, 4344]
    proto = np.array([6, 17, 58, 89])[rng.integers(0, 4, n)]
    buf, dd, groups, n_frag, out_size, od = synth_case(lengths, 1500, 1504, 92, proto=proto, align=rng.integers(0, 16, n),
                                                       out_off=5)
    assert n >= 3072 and n_frag <= 16 * n
    wv, wc, w4, wof, out1 = check(buf, dd, 1500, groups, n_frag, out_size, od, 1504, batch.F_WRITE)
    assert (wv == batch.V_ACCEPT).all() and wc.max() == 4 and wc.min() == 1
    wide = 16 * n + 1
    gv, gc, g4, gof, out4 = gpu_fragment(buf, dd, 1500, groups, wide, out_size, od, 1504, batch.F_WRITE)
    np.testing.assert_array_equal(gv, wv)
    np.testing.assert_array_equal(gc, wc)
    np.testing.assert_array_equal(g4, w4)
    np.testing.assert_array_equal(gof[:n_frag], wof)
    assert (gof["len"][n_frag:] == 0).all()
    np.testing.assert_array_equal(out4, out1)
