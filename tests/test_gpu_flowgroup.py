"""GPU tests of pico_flow_group_batch_dev (picotcp_amd/csrc/pico_csum_k_flow.hip): every case exact against
the restatement (tests/flowgroup_ref.py), with guard elements behind every output array and behind
pico_flow_group_scratch_bytes(n, n_known); then the chains into the gather batches against the
reference-derived fixtures, and one graph capture of grouping + reassembly.

Sizes: the kernels' edges are the wave (64), the parse / probe workgroup (256) and the radix / scan tile
(1024 frames, one a thread), each +-1, and 4099 (five tiles, a second radix pass: 13 key bits)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests import flowgroup_ref as R
from tests.gpu_util import DEV, pairs_dev, replay_captured, to_dev
from tests.test_ref_flowgroup import (check_shape, fixture, flowgroup_known, groups_as_lists, reasm_batch, recovered,
                                      single_key_groups)

pytestmark = pytest.mark.gpu
GUARD = 0xA5
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4099]


def guarded(nbytes: int, dtype, fill=GUARD):
    """(view of nbytes, the whole tensor): 64 guard bytes behind the view."""
    whole = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device=DEV)
    return whole[:nbytes].view(dtype), whole


def run(buf, desc, mode_flags, verdict=None, known=None, seed=0, scratch_fill=0x5A, stream=None):
    """One grouping on the device with guards everywhere; returns host (out_desc, out_index, out_groups,
    counts) in the restatement's layout."""
    n = desc.shape[0]
    nk = 0 if known is None else known.shape[0]
    need = batch.flow_group_scratch_bytes(n, nk)
    assert need > 0 and need % 16 == 0
    od, od_w = guarded(16 * n, torch.uint8)
    oi, oi_w = guarded(4 * n, torch.int32)
    og, og_w = guarded(8 * (n + nk), torch.int32)
    oc, oc_w = guarded(8, torch.int32)
    sc, sc_w = guarded(need, torch.uint8)
    if scratch_fill == "random":
        sc.copy_(to_dev(np.random.default_rng(1).integers(0, 256, need, dtype=np.uint8)))
    else:
        sc.fill_(scratch_fill)
    res = batch.flow_group_batch(to_dev(buf), batch.desc_to_device(desc, DEV), n, mode_flags,
                                 verdict_in=None if verdict is None else to_dev(verdict),
                                 known=None if known is None else to_dev(known.view(np.uint8).reshape(-1)), n_known=nk,
                                 hash_seed=seed, scratch=sc, stream=stream, results=(od, oi, og, oc))
    torch.cuda.synchronize()
    assert res[0] is od
    for name, t, w in (("out_desc", od, od_w), ("out_index", oi, oi_w), ("out_groups", og, og_w), ("out_counts", oc, oc_w),
                       ("scratch", sc, sc_w)):
        assert (w[t.numel() * t.element_size():] == GUARD).all(), f"{name}: a guard byte was written"
    return (od.cpu().numpy().view(R.DESC_DTYPE), oi.cpu().numpy().view(np.uint32),
            og.cpu().numpy().view(np.uint32).reshape(-1, 2), oc.cpu().numpy().view(np.uint32))


def assert_same(got, want, note=""):
    for g, w, name in zip(got, want, ("out_desc", "out_index", "out_groups", "out_counts")):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {note}")


def flow_tuple(f: int):
    """Flow f's (family, src, dst, sport, dport): IPv4 and IPv6 mixed."""
    if f % 3 == 2:
        return 6, bytes([0x20, 1] + [0] * 11 + [f >> 16 & 255, f >> 8 & 255, f & 255]), bytes([0x20, 1] + [0] * 13 + [9]), 1024 + f % 5, 80
    return 4, bytes([10, f >> 16 & 255, f >> 8 & 255, f & 255]), bytes([192, 168, 0, 2]), 1024 + f % 5, 80


def burst(n: int, flows: int, seed: int, eth: bool = False):
    """n frames of `flows` flows in a seeded arrival order (IHL 5 and 7, payloads 0..23): (buf, desc, the
    flow of each frame)."""
    rng = np.random.default_rng(seed)
    who = np.arange(n) if flows >= n else rng.integers(0, flows, n)
    frames = []
    for i, f in enumerate(who):
        fam, src, dst, sp, dp = flow_tuple(int(f))
        fr = R.tcp_frame(fam, src, dst, sp, dp, payload=i % 24, ihl=7 if f % 4 == 1 else 5, fill=i & 255)
        frames.append(R.eth_wrap(fr) if eth else fr)
    buf, desc = R.pack(frames, seed=seed)
    return buf, desc, who


@pytest.mark.parametrize("flows", ["one", "all", "eighth"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(n, flows):
    nf = {"one": 1, "all": n, "eighth": max(1, n // 8)}[flows]
    buf, desc, who = burst(n, nf, seed=n)
    want = R.group(buf, desc, R.FLOW_TCP)
    check_shape(n, 0, *want)
    assert int(want[3][0]) == np.unique(who).size and int(want[3][1]) == n
    assert_same(run(buf, desc, R.FLOW_TCP), want, f"n={n} flows={nf}")


@pytest.mark.parametrize("with_verdict", [False, True])
@pytest.mark.parametrize("eth", [False, True])
def test_variants_and_seeds(eth, with_verdict):
    """IPv4 and IPv6 mixed, IHL > 5, with and without F_ETH and d_verdict_in; identical for every hash seed."""
    n = 1025
    buf, desc, who = burst(n, 97, seed=12, eth=eth)
    verdict = None
    if with_verdict:
        fam6 = np.array([flow_tuple(int(f))[0] == 6 for f in who])
        verdict = np.where(fam6 & eth, R.V_ACCEPT | R.V_IPV6, R.V_ACCEPT).astype(np.uint8)
        verdict[::7] = 4                                    # L4_BAD: not selected
        verdict[5::11] = R.V_FRAG
    mode = R.FLOW_TCP | (R.FLOW_F_ETH if eth else 0)
    want = R.group(buf, desc, mode, verdict)
    check_shape(n, 0, *want)
    assert int(want[3][1]) == (n if verdict is None else int(((verdict & 0x7F) == 1).sum()))
    for seed in (0, 1, 0xFFFFFFFF):
        assert_same(run(buf, desc, mode, verdict, seed=seed), want, f"seed={seed:#x}")


def test_single_group_contention():
    buf, desc, _ = burst(4099, 1, seed=2)
    got = run(buf, desc, R.FLOW_TCP)
    assert list(got[3]) == [1, 4099] and list(got[2][0]) == [0, 4099]
    np.testing.assert_array_equal(got[1], np.arange(4099))
    assert_same(got, R.group(buf, desc, R.FLOW_TCP))


def test_near_miss_keys():
    """Keys that differ in exactly one field each form their own group: sport, dport, one source byte, one
    destination byte, and the family (the IPv4 address bytes repeated in an IPv6 address)."""
    s4, d4 = bytes([10, 1, 2, 3]), bytes([192, 168, 0, 2])
    tuples = [(4, s4, d4, 1000, 80), (4, s4, d4, 1001, 80), (4, s4, d4, 1000, 81), (4, bytes([10, 1, 2, 4]), d4, 1000, 80),
              (4, bytes([11, 1, 2, 3]), d4, 1000, 80), (4, s4, bytes([192, 168, 0, 3]), 1000, 80),
              (4, s4, bytes([192, 169, 0, 2]), 1000, 80), (4, s4, d4, 1000 ^ 0x100, 80), (4, s4, d4, 80, 1000),
              (6, s4 + bytes(12), d4 + bytes(12), 1000, 80), (6, s4 + bytes(11) + b"\1", d4 + bytes(12), 1000, 80),
              (6, s4 + bytes(12), d4 + bytes(11) + b"\1", 1000, 80), (6, s4 + bytes(12), d4 + bytes(12), 1001, 80)]
    rng = np.random.default_rng(6)
    who = np.concatenate([np.arange(len(tuples)), rng.integers(0, len(tuples), 200)])
    frames = [R.tcp_frame(*tuples[int(f)], payload=int(i) % 9, ihl=5 + int(i) % 3) for i, f in enumerate(who)]
    buf, desc = R.pack(frames)
    want = R.group(buf, desc, R.FLOW_TCP)
    assert list(want[3]) == [len(tuples), who.size]
    for t, m in enumerate(groups_as_lists(want[1], want[2], len(tuples))):
        assert m == [int(i) for i in np.where(who == t)[0]]
    assert_same(run(buf, desc, R.FLOW_TCP), want)


def test_unselected_frames():
    """ARP, UDP, a TCP fragment, a frame cut short of its ports, a region past base_len, a wrong verdict:
    in the tail in ascending index, with {0, 0, 0} descriptors."""
    n = 300
    buf, desc, who = burst(n, 11, seed=31, eth=True)
    verdict = np.where(np.array([flow_tuple(int(f))[0] == 6 for f in who]), R.V_ACCEPT | R.V_IPV6, R.V_ACCEPT).astype(np.uint8)
    desc, buf = desc.copy(), buf.copy()
    net = lambda i: int(desc["off"][i]) + 14
    v4 = [i for i in range(n) if flow_tuple(int(who[i]))[0] == 4 and who[i] % 4 != 1]
    arp, udp, frag, cut, past, wrong = v4[3], v4[10], v4[20], v4[30], v4[40], v4[50]
    buf[net(arp) - 2:net(arp)] = [8, 6]
    buf[net(arp):net(arp) + 8] = [0, 1, 8, 0, 6, 4, 0, 1]
    verdict[arp] = 64                                       # V_ARP
    buf[net(udp) + 9] = 17
    buf[net(frag) + 6] = 0x20                               # MF
    verdict[frag] = R.V_FRAG
    desc["len"][cut] = 14 + 20 + 3
    desc["off"][past] = buf.size - 20
    verdict[wrong] = 2                                      # NET_BAD
    out = [arp, udp, frag, cut, past, wrong]
    for vd in (verdict, None):                              # (without verdicts the last is selected: the parse decides)
        want = R.group(buf, desc, R.FLOW_TCP | R.FLOW_F_ETH, vd)
        gone = sorted(out if vd is not None else out[:5])
        nsel = int(want[3][1])
        assert nsel == n - len(gone) and list(want[1][nsel:]) == gone
        assert_same(run(buf, desc, R.FLOW_TCP | R.FLOW_F_ETH, vd), want)
    od = run(buf, desc, R.FLOW_TCP | R.FLOW_F_ETH, verdict)[0]
    assert (od.view(np.uint8).reshape(-1, 16)[n - len(out):] == 0).all()


@pytest.mark.parametrize("nk", [1, 3, 64, 65])
def test_table(nk):
    """Table groups keep table order: empty ones, a duplicate key, frames of known and unknown flows mixed."""
    n, flows = 1500, 90
    buf, desc, who = burst(n, flows, seed=40 + nk)
    # table entry t: flow 2t (present), every fifth an absent flow, entry 2 a duplicate of entry 0
    ids = [1000 + t if t % 5 == 4 else 2 * t for t in range(nk)]
    if nk > 2:
        ids[2] = ids[0]
    known = R.make_known([flow_tuple(f) for f in ids])
    want = R.group(buf, desc, R.FLOW_TCP, known=known)
    check_shape(n, nk, *want)
    lists = groups_as_lists(want[1], want[2], int(want[3][0]))
    for t, f in enumerate(ids):
        dup = nk > 2 and t == 2
        assert lists[t] == ([] if dup else [int(i) for i in np.where(who == f)[0]])
    assert int(want[3][0]) == nk + np.unique(who[~np.isin(who, ids)]).size
    assert_same(run(buf, desc, R.FLOW_TCP, known=known), want, f"nk={nk}")


@pytest.mark.parametrize("fill", [0x00, 0xFF, "random"])
def test_scratch_contents_do_not_matter(fill):
    buf, desc, _ = burst(2049, 300, seed=50)
    known = R.make_known([flow_tuple(f) for f in (7, 8, 2000)])
    assert_same(run(buf, desc, R.FLOW_TCP, known=known, scratch_fill=fill), R.group(buf, desc, R.FLOW_TCP, known=known))


def test_frag_modes_against_restatement():
    """FRAG4 / FRAG6 on synthetic fragments (IPv6 with and without a hop-by-hop header before the fragment
    header), a family the mode does not take mixed in."""
    b4, o4, l4, _ = synth.ipv4_fragments([3000] * 40 + [100] * 5, seed=3)
    d4 = batch.make_desc(o4, l4)
    assert_same(run(b4, d4, R.FLOW_FRAG4), R.group(b4, d4, R.FLOW_FRAG4))
    assert int(run(b4, d4, R.FLOW_FRAG6)[3][1]) == 0
    for hbh in (False, True):
        b6, o6, l6, _ = synth.ipv6_fragments([3000] * 40 + [100] * 5, seed=4, hbh=hbh)
        d6 = batch.make_desc(o6, l6)
        want = R.group(b6, d6, R.FLOW_FRAG6)
        assert int(want[3][1]) > 80
        assert_same(run(b6, d6, R.FLOW_FRAG6), want, f"hbh={hbh}")


def test_wrapper_argument_checks():
    """batch.flow_group_batch refuses what the library would have to trust, before the library is reached."""
    buf, desc, _ = burst(8, 3, seed=1)
    b, d = to_dev(buf), batch.desc_to_device(desc, DEV)
    known = to_dev(R.make_known([flow_tuple(0)]).view(np.uint8).reshape(-1))
    small = torch.zeros(batch.flow_group_scratch_bytes(8, 1) - 1, dtype=torch.uint8, device=DEV)
    for kw in (dict(n=0), dict(n=9), dict(n=1 << 24), dict(n_known=2, known=known), dict(n_known=1), dict(n_known=1, known=known, scratch=small),
               dict(verdict_in=torch.zeros(7, dtype=torch.uint8, device=DEV)), dict(verdict_in=torch.zeros(8, dtype=torch.uint8)),
               dict(results=(torch.zeros(16 * 8, dtype=torch.uint8, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV),
                             torch.zeros(15, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)))):
        args = dict(n=8, mode_flags=R.FLOW_TCP)
        args.update(kw)
        with pytest.raises(ValueError):
            batch.flow_group_batch(b, d, **args)


# ---------------------------------------------------------------- chains into the gather batches

def coalesce_after(buf, desc, conn, cap, od, og, n_conn):
    """tcp_coalesce_batch on the grouping's device-layout results: (verdict, out_len, out bytes, region offsets)."""
    room = (cap.astype(np.int64) + 15) & ~15                           # regions on 16-byte lines
    ooff = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64)
    out = torch.zeros(int(room.sum()) + 16, dtype=torch.uint8, device=DEV)
    v, ol, _ = batch.tcp_coalesce_batch(to_dev(buf), batch.desc_to_device(od, DEV), od.shape[0], pairs_dev(og[:n_conn]),
                                        pairs_dev(conn), out, batch.desc_to_device(batch.make_desc(ooff, cap), DEV))
    torch.cuda.synchronize()
    return v.cpu().numpy(), ol.cpu().numpy().view(np.uint32), out.cpu().numpy(), ooff


def test_chain_tcprx_fixture():
    """Interleaved ref_tcprx_cases -> grouping -> coalescing = the reference's rcv_nxt and read bytes."""
    a = fixture("ref_tcprx_cases.npz")
    arr, perm = synth.interleave_groups(batch.make_desc(a["off"], a["len"]), a["group"], seed=23)
    od, oi, og, counts = run(a["buf"], arr, R.FLOW_TCP)
    assert list(counts) == [24, arr.shape[0]]
    where = recovered(perm, a["group"], range(24), groups_as_lists(oi, og, 24))     # fixture connection -> device group
    assert sorted(where.values()) == list(range(24))
    fix = np.array([g for g, _ in sorted(where.items(), key=lambda kv: kv[1])])     # device group -> fixture connection
    delivered = (a["rcv_after"].astype(np.int64) - a["rcv_before"]) & 0xFFFFFFFF
    conn = np.stack([a["rcv_before"][fix], a["sack_ok"][fix].astype(np.uint32)], axis=1).astype(np.uint32)
    v, ol, out, ooff = coalesce_after(a["buf"], arr, conn, (delivered[fix] + 64).astype(np.uint32), od, og, 24)
    assert (v == 1).all()
    np.testing.assert_array_equal(ol, delivered[fix])
    ro = np.concatenate([[0], np.cumsum(a["read_len"].astype(np.int64))])
    for j, g in enumerate(fix):
        np.testing.assert_array_equal(out[int(ooff[j]):int(ooff[j]) + int(ol[j])], a["read"][ro[g]:ro[g + 1]], err_msg=f"connection {g}")


def test_chain_flowgroup_fixture():
    """ref_flowgroup_cases -> grouping with the 8 tuples as the table -> coalescing = each socket's read
    bytes, by table index: no host step between the two batches."""
    a = fixture("ref_flowgroup_cases.npz")
    desc = batch.make_desc(a["off"], a["len"])
    od, oi, og, counts = run(a["buf"], desc, R.FLOW_TCP, known=flowgroup_known(a))
    assert list(counts) == [8, desc.shape[0]]
    conn = np.stack([a["rcv_before"], a["sack_ok"].astype(np.uint32)], axis=1).astype(np.uint32)
    v, ol, out, ooff = coalesce_after(a["buf"], desc, conn, (a["read_len"] + 64).astype(np.uint32), od, og, 8)
    assert (v == 1).all()
    np.testing.assert_array_equal(ol, a["read_len"])
    np.testing.assert_array_equal(ol, (a["rcv_after"].astype(np.int64) - a["rcv_before"]) & 0xFFFFFFFF)
    ro = np.concatenate([[0], np.cumsum(a["read_len"].astype(np.int64))])
    for t in range(8):
        np.testing.assert_array_equal(out[int(ooff[t]):int(ooff[t]) + int(ol[t])], a["read"][ro[t]:ro[t + 1]], err_msg=f"socket {t}")


@pytest.mark.parametrize("fam", ["v4", "v6"])
def test_chain_reasm_fixture(fam):
    """Interleaved ref_reasm_cases -> grouping -> reassembly = the fixture's bytes, lengths and verdicts on
    the single-key groups (250 IPv4, 265 IPv6: tests/test_ref_flowgroup.py)."""
    a = fixture("ref_reasm_cases.npz")
    buf, arr, perm, groups, keys = reasm_batch(fam)
    od, oi, og, counts = run(buf, arr, R.FLOW_FRAG4 if fam == "v4" else R.FLOW_FRAG6)
    assert_same((od, oi, og, counts), R.group(buf, arr, R.FLOW_FRAG4 if fam == "v4" else R.FLOW_FRAG6))
    ng = int(counts[0])
    single = single_key_groups(groups, keys)
    where = recovered(perm, groups, single, groups_as_lists(oi, og, ng))
    assert None not in where.values() and len(single) == (250 if fam == "v4" else 265)
    ooff, ocap = np.zeros(ng, np.uint64), np.zeros(ng, np.uint32)      # the other groups: no region (MALFORMED)
    for g, j in where.items():
        ooff[j], ocap[j] = a[fam + "_out_off"][g], a[fam + "_out_cap"][g]
    out = torch.zeros(int(a[fam + "_out_size"][0]), dtype=torch.uint8, device=DEV)
    fn = batch.ipv4_reassemble_batch if fam == "v4" else batch.ipv6_reassemble_batch
    ol, l4, v = fn(to_dev(buf), batch.desc_to_device(od, DEV), od.shape[0], pairs_dev(og[:ng]), out,
                   batch.desc_to_device(batch.make_desc(ooff, ocap), DEV))
    torch.cuda.synchronize()
    ol, l4, v, out = ol.cpu().numpy().view(np.uint32), l4.cpu().numpy().view(np.uint16), v.cpu().numpy(), out.cpu().numpy()
    H = 20 if fam == "v4" else 40
    for g, j in where.items():
        assert (v[j], ol[j], l4[j]) == (a[fam + "_verdict"][g], a[fam + "_len"][g], a[fam + "_l4"][g]), f"group {g}"
        if v[j] != 8:
            o, m = int(ooff[j]), H + int(ol[j])
            np.testing.assert_array_equal(out[o:o + m], a[fam + "_exp_out"][o:o + m], err_msg=f"datagram {g}")


def test_graph_capture_with_reassembly():
    """One capture, one stream, no parallel branch: FRAG4 grouping + ipv4_reassemble_batch with a fixed
    n_dgram cap, replayed on two different bursts written into the same buffers."""
    lengths = [3000, 1481, 4000, 100, 2960, 5000, 9, 2000]
    cap = len(lengths) + 3                                              # padded groups: MALFORMED
    bursts = []
    for seed in (61, 62):
        b, o, ln, g = synth.ipv4_fragments(lengths, seed=seed)
        arr, _ = synth.interleave_groups(batch.make_desc(o, ln), g, seed=seed)
        bursts.append((b, arr))
    n = bursts[0][1].shape[0]
    assert bursts[1][1].shape[0] == n and bursts[0][0].size == bursts[1][0].size
    base, desc = to_dev(bursts[0][0]), batch.desc_to_device(bursts[0][1], DEV)
    region = 20 + max(lengths) + 16
    outd = batch.make_desc(12 + 16 * ((region + 15) // 16) * np.arange(cap), np.full(cap, region))
    out = torch.zeros(16 * ((region + 15) // 16) * cap + 32, dtype=torch.uint8, device=DEV)
    outd_t = batch.desc_to_device(outd, DEV)
    od = torch.zeros(16 * n, dtype=torch.uint8, device=DEV)
    oi, og, oc = (torch.zeros(k, dtype=torch.int32, device=DEV) for k in (n, 2 * n, 2))
    scratch = torch.zeros(batch.flow_group_scratch_bytes(n), dtype=torch.uint8, device=DEV)
    res = tuple(torch.zeros(cap, dtype=dt, device=DEV) for dt in (torch.int32, torch.int16, torch.uint8))
    state = {"k": 0}

    def call(s):
        batch.flow_group_batch(base, desc, n, R.FLOW_FRAG4, scratch=scratch, stream=s, results=(od, oi, og, oc))
        batch.ipv4_reassemble_batch(base, od, n, og[:2 * cap], out, outd_t, stream=s, results=res)

    def reset():
        b, arr = bursts[state["k"]]
        base.copy_(torch.from_numpy(b.copy()))
        desc.copy_(torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()))
        out.zero_()

    def check():
        b, arr = bursts[state["k"]]
        state["k"] += 1
        want = R.group(b, arr, R.FLOW_FRAG4)
        got = (od.cpu().numpy().view(R.DESC_DTYPE), oi.cpu().numpy().view(np.uint32),
               og.cpu().numpy().view(np.uint32).reshape(-1, 2), oc.cpu().numpy().view(np.uint32))
        assert_same(got, want, f"replay {state['k']}")
        ng = int(want[3][0])
        assert ng == len(lengths) - 2                       # (the 9- and 100-byte datagrams: one frame, no MF, not a fragment)
        ref_out = np.zeros(out.numel(), np.uint8)
        wl, w4, wv = O.ipv4_reassemble(b, want[0], want[2][:ng], ref_out, outd[:ng])
        np.testing.assert_array_equal(res[2].cpu().numpy()[:ng], wv)
        np.testing.assert_array_equal(res[0].cpu().numpy().view(np.uint32)[:ng], wl)
        np.testing.assert_array_equal(res[1].cpu().numpy().view(np.uint16)[:ng], w4)
        assert (res[2].cpu().numpy()[ng:] == 8).all() and (wv == 1).sum() >= 5
        o = out.cpu().numpy()
        for g in np.flatnonzero(wv != 8):
            a0, m = int(outd["off"][g]), 20 + int(wl[g])
            np.testing.assert_array_equal(o[a0:a0 + m], ref_out[a0:a0 + m], err_msg=f"datagram {g}")

    replay_captured(call, reset, check, times=2)
