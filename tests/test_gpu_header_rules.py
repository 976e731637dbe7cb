"""GPU: the protocols' header rules (eth_classify / ipv4_classify / ipv6_dispatch / nat_stage in
pico_csum_k_sorted.hip) on both paths of the fused kernel.  One burst of 512 small frames in which
every rule's edge occurs at least 4 times is laid out twice -- back to back with 0-3 byte gaps and
odd starts (stream-order waves) and one frame per 4 KiB slot (sorted rounds) -- and run at 64 and
4 frames per wave: every output must equal the oracle's, and so each layout's the other's; the
bytes NAT writes must equal the bytes the oracle wrote, and the TX checksums must be stored where
include/pico_csum.h says (the oracle's values; it has no write-back of its own for those modes).
Frames that send a whole wave to the sorted rounds (IPv4 options, a crc field or bytes past the
datagram beyond the 64-byte head window, IPv6 extension headers, an IPv6 seed) sit in the last 64
positions only, so the other waves of the dense layout stay on the stream (check_coverage asserts
it from the descriptors).  Frames are 40-200 bytes but for the 14-byte Ethernet frame."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests.test_gpu_parity import to_dev

N, TAIL = 512, 64
MAC = bytes.fromhex("02005e0a0b0c")
ACCEPT, NET_BAD, L4_BAD, MALFORMED = batch.V_ACCEPT, 2, 4, 8

V4_KINDS = ("tcp", "udp", "icmp", "udp_crc0", "tot_over", "ihl4", "evil", "src_bcast", "src_mcast", "src_loop", "mf",
            "offset", "udp_short", "tcp_short", "icmp_short", "l4_bad", "net_bad", "other", "icmp_opt")
V4_TAIL = ("opt_tcp", "opt_udp", "tail", "udp")
V6_KINDS = ("tcp", "udp", "icmp128", "icmp135", "tcp_b9_17", "tcp_b9_6", "udp_b9_17", "udp_crc0", "udp_short",
            "icmp_empty", "icmp_empty_tail", "tcp_short", "l4_bad", "icmp135_bad", "icmp128_bad")
V6_TAIL = ("hbh_seed", "hbh_walk", "dst_walk", "frag")
DST = (MAC, b"\xff" * 6, bytes([0x01, 0x00, 0x5e, 1, 2, 3]), bytes([0x33, 0x33, 0, 0, 0, 1]),
       bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55]))
DST_NAMES = ("own", "broadcast", "mcast4", "mcast6", "foreign")
ETH_EDGES = {0: "arp", 1: "ethertype", 2: "bare", 3: "version"}      # by i % 29, else an IP frame


def kinds(names, tail):
    return [names[i % len(names)] if i < N - TAIL else tail[i % len(tail)] for i in range(N)]


def put16(f, pos, val):
    f[pos], f[pos + 1] = (val >> 8) & 0xFF, val & 0xFF


def pack(frames):
    """Frames back to back: (buffer, descriptors)."""
    lens = np.array([f.size for f in frames], np.uint32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return np.concatenate(frames), batch.make_desc(off, lens)


def v4_frames():
    """IPv4 datagrams (descriptor at the IP header) with valid checksums but for the edge named by
    their kind."""
    rng = np.random.default_rng(41)
    kind, frames = kinds(V4_KINDS, V4_TAIL), []
    for i, k in enumerate(kind):
        proto = {"udp": 17, "udp_crc0": 17, "udp_short": 17, "opt_udp": 17, "icmp": 1, "icmp_short": 1,
                 "icmp_opt": 1, "other": 47}.get(k, 6)
        # the short transports sit behind options that end inside the head window: 40-byte datagrams
        ihl = {"opt_tcp": 15, "opt_udp": 15, "udp_short": 9, "icmp_short": 9, "tcp_short": 7, "icmp_opt": 6}.get(k, 5)
        ln = int(rng.integers(96 if ihl == 15 else 48 if k == "tail" else 40, 187))
        if k in ("udp_short", "icmp_short", "tcp_short"):
            ln = 48
        f, _, _ = synth.ipv4_batch(np.array([ln], np.uint32), seed=1000 + i, proto=proto, eth=False, ihl=ihl)
        if k == "udp_short":
            f = f[:40 + i % 4].copy()
            put16(f, 2, f.size)
        elif k == "tot_over":
            put16(f, 2, ln + 4)
        elif k == "ihl4":
            f[0] = 0x44
        elif k == "evil":
            f[6] |= 0x80
        elif k == "src_bcast":
            f[12:16] = 255
        elif k == "src_mcast":
            f[12] = 224 + i % 31
        elif k == "src_loop":
            f[12] = 127
        elif k == "mf":
            f[6], f[7] = 0x20, 0
        elif k == "offset":
            f[6], f[7] = 0, 0x10
        elif k in ("tcp_short", "icmp_short"):       # 12 of TCP's 20 bytes, 4 of ICMP's 8
            f = f[:40].copy()
            put16(f, 2, 40)
        elif k == "tail":
            put16(f, 2, ln - 5)
        frames.append(f)
    buf, desc = pack(frames)
    wn, wl, wv = O.batch_ipv4(buf, desc, tx=True)
    for i, (f, k) in enumerate(zip(frames, kind)):
        if wn[i] == 0:                    # the lengths do not fit: no header checksum
            continue
        put16(f, 10, int(wn[i]))
        hl = 20 + 4 * max((int(f[0]) & 15) - 5, 0)
        tl = ((int(f[2]) << 8 | int(f[3])) - hl) & 0xFFFF
        if wv[i] == ACCEPT and f[9] in (6, 1):
            put16(f, hl + (16 if f[9] == 6 else 2), int(wl[i]))
        elif wv[i] == ACCEPT and f[9] == 17 and tl >= 8 and k != "udp_crc0":
            ph = np.concatenate([f[12:20], np.array([0, 17, tl >> 8, tl & 0xFF], np.uint8)])
            put16(f, hl + 6, O.dualbuffer_checksum(ph, f[hl:hl + tl]) or 0xFFFF)
        if k == "l4_bad":
            f[hl + 4] ^= 0x40
        elif k == "net_bad":
            f[8] ^= 1
    nat = np.zeros(N, O.NAT_DTYPE)
    nat["addr"] = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    nat["port"] = rng.integers(0, 1 << 16, N).astype(np.uint16)
    nat["dir"] = (np.arange(N) // len(V4_KINDS)) % 3          # every kind meets every direction
    return frames, kind, nat


def v6_frames():
    """IPv6 datagrams (descriptor at the IPv6 header, seed 0 unless the kind says otherwise)."""
    rng = np.random.default_rng(61)
    kind, frames, seeds = kinds(V6_KINDS, V6_TAIL), [], np.zeros(N, np.uint32)
    for i, k in enumerate(kind):
        proto = 17 if k.startswith("udp") else 58 if k.startswith("icmp") else 6
        ext = i >= N - TAIL
        ln = 40 + 8 * int(rng.integers(4, 18)) if ext else int(rng.integers(60, 187))
        if k in ("udp_short", "icmp_empty", "icmp_empty_tail"):
            ln = 48
        f, _, _, sd = synth.ipv6_batch(np.array([ln], np.uint32), seed=2000 + i, proto=proto, eth=False,
                                       hbh=k.startswith("hbh"), destopt=k == "dst_walk",
                                       icmp_type=135 if k.startswith("icmp135") else 128,
                                       frag=(i % 50) << 3 | (i >> 2 & 1) if k == "frag" else None, walked=k != "hbh_seed")
        seeds[i] = sd[0]
        if k in ("tcp_b9_17", "udp_b9_17"):
            f[9] = 17
        elif k == "tcp_b9_6":
            f[9] = 6
        elif f[9] in (6, 17):             # every other kind: a byte 9 the reference does not dispatch on
            f[9] = 99
        if k == "tcp_short":              # 12 of TCP's 20 bytes
            f = f[:52].copy()
            put16(f, 4, 12)
        elif k == "udp_short":            # 4-7 transport bytes
            f = f[:44 + i % 4].copy()
            put16(f, 4, f.size - 40)
        elif k in ("icmp_empty", "icmp_empty_tail"):      # no transport byte; 4 bytes past the datagram
            f = f[:40 if k == "icmp_empty" else 44].copy()
            put16(f, 4, 0)
        frames.append(f)
    buf, desc = pack(frames)
    txd = desc.copy()                 # TX takes the transport behind the extension headers from the seed
    txd["seed"][N - TAIL:] = 48 | 6 << 16
    wl, wv = O.batch_ipv6(buf, txd, tx=True)
    for i, (f, k) in enumerate(zip(frames, kind)):
        t = 48 if i >= N - TAIL else 40
        nh = int(f[t - 8]) if t == 48 else int(f[6])
        if wv[i] == ACCEPT and nh in (6, 17, 58) and k != "udp_crc0":
            put16(f, t + {6: 16, 17: 6, 58: 2}[nh], int(wl[i]))
        if k in ("l4_bad", "icmp135_bad", "icmp128_bad"):
            f[t + 5] ^= 0x40
    return frames, kind, seeds


def eth_frames(v4, v6, seeds6):
    """Ethernet frames: the IPv4 (even positions) and IPv6 (odd) datagrams behind a 14-byte header
    whose destination cycles through DST, and every 29th position one of ETH_EDGES."""
    frames, kind, seeds = [], [], np.zeros(N, np.uint32)
    for i in range(N):
        ip, et = (v4[i], 0x0800) if i % 2 == 0 else (v6[i], 0x86DD)
        edge = ETH_EDGES.get(i % 29)
        dst = DST[0] if edge else DST[(i // 2) % len(DST)]
        if edge == "arp":
            ip, et = synth.random_bytes(3000 + i, 46), 0x0806
        elif edge == "ethertype":
            et = 0x88CC
        elif edge == "bare":
            ip = ip[:0]
        elif edge == "version":
            et ^= 0x0800 ^ 0x86DD
        hdr = np.concatenate([np.frombuffer(dst, np.uint8), synth.random_bytes(4000 + i, 6),
                              np.array([et >> 8, et & 0xFF], np.uint8)])
        frames.append(np.concatenate([hdr, ip]))
        kind.append(edge or DST_NAMES[(i // 2) % len(DST)] + ("_v4" if i % 2 == 0 else "_v6"))
        seeds[i] = seeds6[i] if i % 2 and edge is None else 0
    return frames, kind, seeds


def head_reach(f, l2=0, v6=False, tx=True):
    """How many bytes from the frame's start the stream's finish takes from the frame's head window
    (64 bytes from the start's 16-byte line; past it the wave falls back to the sorted rounds): an
    IPv4 datagram's options, its crc field and any bytes behind the datagram; an IPv6 batch's bytes
    behind the datagram.  0: none.  tx: the burst also runs TX and NAT (their TCP / ICMP fields)."""
    ip = f[l2:]
    if v6:
        return f.size if 40 + (int(ip[4]) << 8 | int(ip[5])) < ip.size else 0
    if ip.size < 20 or ip[0] >> 4 != 4 or (l2 and (f[12], f[13]) != (0x08, 0x00)):
        return 0
    hl = 20 + 4 * max((int(ip[0]) & 15) - 5, 0)
    tl = ((int(ip[2]) << 8 | int(ip[3])) - hl) & 0xFFFF
    field = {6: 18 if tx else 0, 17: 8, 1: 4 if tx else 0}.get(int(ip[9]), 0)
    return f.size if hl + tl < ip.size else l2 + hl + (field if tl >= field else 0)


def lay_out(frames, how, seed, seeds=None, reach=None):
    """'dense': back to back, 0-3 byte gaps (one more where a frame's head_reach would otherwise
    leave its head window), odd starts among them; 'sparse': one frame per 4 KiB slot, 0-15 bytes
    into it."""
    rng = np.random.default_rng(seed)
    lens = np.array([f.size for f in frames], np.int64)
    if how == "dense":
        off, pos = np.zeros(N, np.int64), 1
        for i, g in enumerate(rng.integers(0, 4, N)):
            pos += int(g)
            if i < N - TAIL and reach[i] <= 64 < (pos & 15) + reach[i]:
                pos += 1
            off[i] = pos
            pos += int(lens[i])
    else:
        off = np.arange(N, dtype=np.int64) * 4096 + rng.integers(0, 16, N)
    buf = synth.random_bytes(seed, int(off[-1] + lens[-1]) + 64)
    for o, f in zip(off, frames):
        buf[o:o + f.size] = f
    return buf, batch.make_desc(off.astype(np.uint64), lens.astype(np.uint32), seeds)


def stored_v4(buf, desc, wn, wl, wv):
    """What F_TX | F_WRITE leaves (include/pico_csum.h): accepted frames get the header checksum
    and the TCP / ICMP checksum, UDP its crc 0; a fragment its header checksum only."""
    out = buf.copy()
    for o, n, l4, v in zip(desc["off"].astype(np.int64), wn, wl, wv):
        if v in (ACCEPT, batch.V_FRAG):
            put16(out, o + 10, int(n))
        hl = 20 + 4 * max((int(buf[o]) & 15) - 5, 0)
        tl = ((int(buf[o + 2]) << 8 | int(buf[o + 3])) - hl) & 0xFFFF
        if v == ACCEPT and buf[o + 9] in (6, 1):
            put16(out, o + hl + (16 if buf[o + 9] == 6 else 2), int(l4))
        elif v == ACCEPT and buf[o + 9] == 17 and tl >= 8:
            put16(out, o + hl + 6, 0)
    return out


def stored_v6(buf, desc, wl, wv):
    out = buf.copy()
    for o, sd, l4, v in zip(desc["off"].astype(np.int64), desc["seed"], wl, wv):
        nl, nh = (int(sd) & 0xFFFF, int(sd) >> 16) if sd else (40, int(buf[o + 6]))
        if v == ACCEPT and nh in (6, 17, 58):
            put16(out, o + nl + {6: 16, 17: 6, 58: 2}[nh], int(l4))
    return out


@functools.lru_cache(maxsize=None)
def burst():
    """The frames, both layouts of each family, and the oracle's answers (computed once)."""
    v4, k4, nat = v4_frames()
    v6, k6, s6 = v6_frames()
    eth, ke, se = eth_frames(v4, v6, s6)
    b = dict(k4=k4, k6=k6, ke=ke, nat=nat, reach4=[head_reach(f) for f in v4],
             reach6=[head_reach(f, v6=True) for f in v6], reache=[head_reach(f, 14, tx=False) for f in eth])
    for how, seed in (("dense", 7), ("sparse", 8)):
        w = b[how] = {}
        buf, desc = w["v4"] = lay_out(v4, how, seed, reach=b["reach4"])
        w["v4_rx"] = O.batch_ipv4(buf, desc)
        w["v4_tx"] = O.batch_ipv4(buf, desc, tx=True)
        w["v4_stored"] = stored_v4(buf, desc, *w["v4_tx"])
        w["nat_stored"] = buf.copy()
        w["nat"] = O.batch_ipv4_nat(w["nat_stored"], desc, nat)
        buf, desc = w["v6"] = lay_out(v6, how, seed + 10, s6, reach=b["reach6"])
        w["v6_rx"] = O.batch_ipv6(buf, desc)
        w["v6_nxd"] = O.batch_ipv6(buf, desc, nxthdr_dispatch=True)
        w["v6_tx"] = O.batch_ipv6(buf, desc, tx=True)
        w["v6_stored"] = stored_v6(buf, desc, *w["v6_tx"])
        buf, desc = w["eth"] = lay_out(eth, how, seed + 20, se, reach=b["reache"])
        w["eth_rx"] = O.batch_eth(buf, desc, mac=MAC)
    return b


@functools.lru_cache(maxsize=None)
def check_coverage():
    """Every edge the helpers decide is in the burst at least 4 times, by the oracle's verdicts."""
    b = burst()
    w = b["dense"]
    k4, k6, ke = np.array(b["k4"]), np.array(b["k6"]), np.array(b["ke"])

    def every(sel, verdicts, want, what):
        assert sel.sum() >= 4 and (verdicts[sel] == want).all(), what

    n4, l4, rx = w["v4_rx"]
    for k in ("tcp", "udp", "icmp", "udp_crc0", "other", "tail", "icmp_short", "icmp_opt", "opt_tcp", "opt_udp"):
        every(k4 == k, rx, ACCEPT, k)
    for k in ("tot_over", "udp_short"):
        every(k4 == k, rx, MALFORMED, k)
    for k in ("ihl4", "evil", "src_bcast", "src_mcast", "src_loop"):       # dropped behind a valid header
        every(k4 == k, rx, MALFORMED, k)
        assert (n4[k4 == k] == 0).all(), k
    every((k4 == "mf") | (k4 == "offset"), rx, batch.V_FRAG, "fragments")
    every(k4 == "l4_bad", rx, L4_BAD, "l4_bad")
    every(k4 == "net_bad", rx, NET_BAD, "net_bad")
    assert (l4[(k4 == "udp_crc0")] == 0).all() and (l4[k4 == "udp"] == 0).all()
    tx = w["v4_tx"][2]
    for k in ("tcp_short", "icmp_short", "tot_over"):
        every(k4 == k, tx, MALFORMED, "tx " + k)
    for k in ("tcp", "udp", "icmp", "ihl4", "evil", "src_loop"):
        every(k4 == k, tx, ACCEPT, "tx " + k)
    every((k4 == "mf") | (k4 == "offset"), tx, batch.V_FRAG, "tx fragments")
    nv, d = w["nat"][2], b["nat"]["dir"]
    for k in ("tcp", "udp", "icmp"):
        every((k4 == k) & (d == 0), nv, batch.V_UNTOUCHED, "nat none " + k)
        for dr in (1, 2):
            every((k4 == k) & (d == dr), nv, ACCEPT, f"nat {dr} {k}")
    for k in ("tcp_short", "udp_short"):
        every((k4 == k) & (d != 0), nv, MALFORMED, "nat " + k)
    every((k4 == "mf") | (k4 == "offset"), nv, batch.V_FRAG, "nat fragments")
    every((k4 == "other") & (d != 0), nv, batch.V_UNTOUCHED, "nat other")

    (l6, rx), (ln, nx), (_, tx) = w["v6_rx"], w["v6_nxd"], w["v6_tx"]
    for k in ("tcp", "udp", "icmp128", "icmp135", "tcp_b9_6", "udp_b9_17", "udp_crc0", "icmp_empty_tail",
              "icmp128_bad", "hbh_seed", "hbh_walk", "dst_walk"):
        every(k6 == k, rx, ACCEPT, k)
        every(k6 == k, nx, ACCEPT, k + " nxd")
    every(k6 == "tcp_b9_17", rx, L4_BAD, "byte 9 = 17 on TCP, the reference's dispatch")
    every(k6 == "tcp_b9_17", nx, ACCEPT, "byte 9 = 17 on TCP, next-header dispatch")
    for k in ("udp_short", "icmp_empty"):
        every(k6 == k, rx, MALFORMED, k)
        every(k6 == k, nx, MALFORMED, k + " nxd")
        every(k6 == k, tx, MALFORMED, k + " tx")
    every(k6 == "tcp_short", tx, MALFORMED, "tx tcp_short")
    every(k6 == "icmp135_bad", rx, L4_BAD, "icmp135_bad")
    every(k6 == "l4_bad", nx, L4_BAD, "l4_bad nxd")
    every(k6 == "frag", rx, batch.V_FRAG, "ipv6 fragment header")
    assert (l6[k6 == "icmp128_bad"] != 0).all() and (ln[k6 == "udp"] == 0).all()
    assert (w["v6"][1]["seed"][k6 == "hbh_seed"] != 0).all() and (w["v6"][1]["seed"][k6 != "hbh_seed"] == 0).all()

    ev = w["eth_rx"][2]
    every(np.char.startswith(ke, "foreign"), ev, batch.V_DROP_L2, "foreign unicast")
    every(ke == "arp", ev, batch.V_ARP, "arp")
    every(ke == "ethertype", ev, batch.V_DROP_L2, "unknown ethertype")
    every(ke == "version", ev, batch.V_DROP_L2, "ethertype / version mismatch")
    every(ke == "bare", ev, MALFORMED, "no IP byte")
    for name in ("own", "broadcast", "mcast4", "mcast6"):
        every((ke == name + "_v4") & (w["v4_rx"][2] == ACCEPT), ev, ACCEPT, name)
        every((ke == name + "_v6") & (rx == ACCEPT), ev, ACCEPT | batch.V_IPV6, name + " v6")
    seen = set(np.concatenate([w[m][-1] for m in ("v4_rx", "v4_tx", "nat", "v6_rx", "v6_nxd", "v6_tx", "eth_rx")]))
    assert {ACCEPT, NET_BAD, L4_BAD, MALFORMED, batch.V_FRAG, batch.V_DROP_L2, batch.V_ARP, batch.V_UNTOUCHED,
            ACCEPT | batch.V_IPV6, MALFORMED | batch.V_IPV6} <= seen
    # the dense layout's waves before the last 64 positions stay on the stream: nothing the finish
    # takes from a head window lies past it, no IPv6 walk, no seed
    body = slice(0, N - TAIL)
    for fam in ("4", "6", "e"):
        desc = w["v" + fam if fam != "e" else "eth"][1]
        assert ((desc["off"][body] & 15) + np.array(b["reach" + fam])[body] <= 64).all(), fam
    nh = np.array([w["v6"][0][int(o) + 6] for o in w["v6"][1]["off"][body]])
    assert np.isin(nh, (6, 17, 58)).all() and (w["v6"][1]["seed"][body] == 0).all()
    assert (w["eth"][1]["seed"][body] == 0).all()
    for k, reach in (("opt_tcp", b["reach4"]), ("opt_udp", b["reach4"]), ("tail", b["reach4"])):
        assert (np.array(reach)[k4 == k] > 64 - 15).all(), k      # these can leave the window
    for how in ("dense", "sparse"):                   # what each layout is for
        span = b[how]["v4"][1]
        ends = (span["off"] + span["len"]).astype(np.int64)
        assert (int(ends[63]) - int(span["off"][0]) <= 2 * int(span["len"][:64].sum()) + 4096) == (how == "dense")
    assert (b["dense"]["v4"][1]["off"] & 1).any() and (b["dense"]["eth"][1]["off"] & 1).any()


def test_burst_covers_every_edge():
    check_coverage()


@pytest.fixture(autouse=True)
def _reset_override():
    yield
    batch.set_launch_override(0)


def np16(t):
    return t.cpu().numpy().view(np.uint16)


def both_layouts(run, want_key):
    """run(layout) -> outputs; each layout's must equal the oracle's, and so each other's."""
    got = {}
    for how in ("dense", "sparse"):
        w = burst()[how]
        got[how] = run(w)
        for g, want in zip(got[how], w[want_key]):
            np.testing.assert_array_equal(g, want, err_msg=f"{how} {want_key}")
    for a, c in zip(got["dense"], got["sparse"]):
        np.testing.assert_array_equal(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("fpw", [64, 4])
def test_ipv4_rules(fpw):
    check_coverage()
    batch.set_launch_override(2, fpw=fpw)

    def rx(w):
        buf, desc = w["v4"]
        n, l4, v = batch.ipv4_checksum_batch(to_dev(buf), batch.desc_to_device(desc, "cuda:0"), N)
        torch.cuda.synchronize()
        return np16(n), np16(l4), v.cpu().numpy()

    def tx(w):
        buf, desc = w["v4"]
        d = to_dev(buf)
        n, l4, v = batch.ipv4_checksum_batch(d, batch.desc_to_device(desc, "cuda:0"), N,
                                             flags=batch.F_TX | batch.F_WRITE)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d.cpu().numpy(), w["v4_stored"])
        return np16(n), np16(l4), v.cpu().numpy()

    both_layouts(rx, "v4_rx")
    both_layouts(tx, "v4_tx")


@pytest.mark.gpu
@pytest.mark.parametrize("fpw", [64, 4])
def test_ipv6_rules(fpw):
    check_coverage()
    batch.set_launch_override(2, fpw=fpw)

    def run(flags, stored=None):
        def go(w):
            buf, desc = w["v6"]
            d = to_dev(buf)
            l4, v = batch.ipv6_checksum_batch(d, batch.desc_to_device(desc, "cuda:0"), N, flags=flags)
            torch.cuda.synchronize()
            if stored:
                np.testing.assert_array_equal(d.cpu().numpy(), w[stored])
            return np16(l4), v.cpu().numpy()
        return go

    both_layouts(run(0), "v6_rx")
    both_layouts(run(batch.F_NXTHDR_DISPATCH), "v6_nxd")
    both_layouts(run(batch.F_TX | batch.F_WRITE, "v6_stored"), "v6_tx")


@pytest.mark.gpu
@pytest.mark.parametrize("fpw", [64, 4])
def test_eth_rules(fpw):
    check_coverage()
    batch.set_launch_override(2, fpw=fpw)

    def rx(w):
        buf, desc = w["eth"]
        n, l4, v = batch.eth_checksum_batch(to_dev(buf), batch.desc_to_device(desc, "cuda:0"), N, mac=MAC)
        torch.cuda.synchronize()
        return np16(n), np16(l4), v.cpu().numpy()

    both_layouts(rx, "eth_rx")


@pytest.mark.gpu
@pytest.mark.parametrize("fpw", [64, 4])
def test_nat_rules(fpw):
    check_coverage()
    batch.set_launch_override(2, fpw=fpw)

    def nat(w):
        buf, desc = w["v4"]
        d = to_dev(buf)
        n, l4, v = batch.ipv4_nat_batch(d, batch.desc_to_device(desc, "cuda:0"), N,
                                        to_dev(burst()["nat"].view(np.uint8)))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d.cpu().numpy(), w["nat_stored"])
        return np16(n), np16(l4), v.cpu().numpy()

    both_layouts(nat, "nat")
