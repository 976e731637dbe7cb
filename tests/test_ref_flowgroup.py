"""The restatement of pico_flow_group_batch_dev's contract (tests/flowgroup_ref.py) on bursts whose true
groups are known (no GPU): synthetic bursts, the two reference-derived fixtures of the gather batches
with their groups interleaved, and tests/golden/ref_flowgroup_cases.npz
(tests/golden/make_ref_flowgroup.py), which pins the TCP key to the compiled reference stack's
pico_socket_tcp_deliver: 8 connections with near-miss tuples, their segments injected interleaved, the
bytes every child socket read.  tests/test_gpu_flowgroup.py checks the kernels against the
restatement and against the same fixtures."""
from __future__ import annotations

import os

import numpy as np
import pytest

from picotcp_amd import _lib, batch, synth
from tests import flowgroup_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache: dict = {}


def fixture(name: str):
    """A fixture's arrays (loaded once, shared, read-only)."""
    if name not in _cache:
        c = np.load(os.path.join(GOLDEN, name))
        _cache[name] = {k: c[k] for k in c.files}
        for a in _cache[name].values():
            a.setflags(write=False)
    return _cache[name]


def groups_as_lists(oi, og, n_groups):
    """out_groups / out_index as one list of input indexes per group."""
    return [[int(i) for i in oi[int(f):int(f) + int(c)]] for f, c in og[:n_groups]]


def check_shape(n, nk, od, oi, og, counts):
    """What holds for every result: a permutation, groups that tile the selected slots in order, zero
    padding, the unselected tail ascending."""
    ng, nsel = int(counts[0]), int(counts[1])
    assert sorted(int(i) for i in oi) == list(range(n))
    assert nk <= ng <= n + nk and nsel <= n
    assert (og[ng:] == 0).all()
    pos = 0
    for g, (f, c) in enumerate(og[:ng]):
        if c == 0:
            assert g < nk and f == 0                        # only a table group may be empty
            continue
        assert f == pos
        assert list(oi[f:f + c]) == sorted(oi[f:f + c])     # arrival order
        pos += int(c)
    assert pos == nsel
    assert list(oi[nsel:]) == sorted(oi[nsel:])
    assert (od["off"][nsel:] == 0).all() and (od["len"][nsel:] == 0).all() and (od["seed"] == 0).all()
    firsts = [int(oi[f]) for f, c in og[nk:ng]]
    assert firsts == sorted(firsts)                         # unknown groups by first arrival


def reasm_batch(fam: str):
    """The reassembly fixture's fragments of one family, interleaved: (buf, desc in arrival order, perm,
    the fixture's groups, each fragment's key or None, in fixture order)."""
    key = ("reasm", fam)
    if key not in _cache:
        a = fixture("ref_reasm_cases.npz")
        mode = R.FLOW_FRAG4 if fam == "v4" else R.FLOW_FRAG6
        desc = batch.make_desc(a[fam + "_frag_off"], a[fam + "_frag_len"])
        keys = [R.frame_key(a[fam + "_buf"], int(o), int(ln), mode) for o, ln in zip(desc["off"], desc["len"])]
        arr, perm = synth.interleave_groups(desc, a[fam + "_groups"], seed=17)
        _cache[key] = (a[fam + "_buf"], arr, perm, a[fam + "_groups"], [None if k is None else k[0] for k in keys])
    return _cache[key]


def single_key_groups(groups, keys):
    """The fixture groups every member of which is selected and carries one key."""
    return [g for g, (f, c) in enumerate(groups) if c and None not in keys[f:f + c] and len(set(keys[f:f + c])) == 1]


def recovered(perm, groups, which, got_lists):
    """Fixture group -> the restated (or device) group that holds exactly its members, in its order."""
    inv = np.empty(perm.size, np.int64)
    inv[perm] = np.arange(perm.size)
    by_members = {tuple(m): j for j, m in enumerate(got_lists)}
    out = {}
    for g in which:
        f, c = groups[g]
        out[g] = by_members.get(tuple(int(inv[i]) for i in range(f, f + c)))
    return out


# ---------------------------------------------------------------- synthetic bursts

def synth_burst(n_flows: int, per_flow, seed: int, eth: bool = False):
    """n_flows TCP flows (IPv4 and IPv6 mixed, IHL 5 and 7) of per_flow frames each, group-contiguous."""
    rng = np.random.default_rng(seed)
    frames, groups = [], []
    for f in range(n_flows):
        fam = 6 if f % 3 == 2 else 4
        src = bytes([10, f >> 8 & 255, f & 255, 1]) if fam == 4 else bytes([0x20, 1] + [0] * 12 + [f >> 8 & 255, f & 255])
        dst = bytes([192, 168, 0, 2]) if fam == 4 else bytes([0x20, 1] + [0] * 13 + [9])
        cnt = int(per_flow if np.isscalar(per_flow) else per_flow[f])
        groups.append((len(frames), cnt))
        for _ in range(cnt):
            fr = R.tcp_frame(fam, src, dst, 1024 + f % 7, 80, payload=int(rng.integers(0, 40)), ihl=7 if f % 4 == 1 else 5,
                             fill=int(rng.integers(256)))
            frames.append(R.eth_wrap(fr) if eth else fr)
    return frames, np.array(groups, np.uint32)


@pytest.mark.parametrize("n_flows,per_flow,eth", [(1, 9, False), (9, 1, True), (12, 5, False), (12, 5, True)])
def test_synthetic_groups_are_recovered(n_flows, per_flow, eth):
    frames, groups = synth_burst(n_flows, per_flow, seed=3, eth=eth)
    buf, desc = R.pack(frames)
    arr, perm = synth.interleave_groups(desc, groups, seed=4)
    assert sorted(perm) == list(range(len(frames)))
    for f, c in groups:                                     # the merge keeps each group's order
        where = [int(np.where(perm == i)[0][0]) for i in range(f, f + c)]
        assert where == sorted(where)
    od, oi, og, counts = R.group(buf, arr, R.FLOW_TCP | (R.FLOW_F_ETH if eth else 0))
    check_shape(len(frames), 0, od, oi, og, counts)
    assert list(counts) == [n_flows, len(frames)]
    got = recovered(perm, groups, range(n_flows), groups_as_lists(oi, og, int(counts[0])))
    assert None not in got.values() and len(set(got.values())) == n_flows
    skip = 14 if eth else 0
    np.testing.assert_array_equal(od["off"], arr["off"][oi] + skip)
    np.testing.assert_array_equal(od["len"], arr["len"][oi] - skip)


def test_table_groups_keep_table_order():
    frames, groups = synth_burst(6, 3, seed=8)
    buf, desc = R.pack(frames)
    arr, perm = synth.interleave_groups(desc, groups, seed=9)
    key = lambda f: R.frame_key(buf, int(desc["off"][groups[f][0]]), int(desc["len"][groups[f][0]]), R.FLOW_TCP)[0]
    known = np.zeros(4, R.FLOW_KEY_DTYPE)
    for t, k in enumerate((key(4), (4, bytes(16), bytes(16), b"\0\0\0\0"), key(1), key(4))):   # flow 4, no frame's, flow 1, a duplicate
        known["family"][t] = k[0]
        known["src"][t], known["dst"][t] = np.frombuffer(k[1], np.uint8), np.frombuffer(k[2], np.uint8)
        known["sport"][t], known["dport"][t] = int.from_bytes(k[3][:2], "little"), int.from_bytes(k[3][2:], "little")
    od, oi, og, counts = R.group(buf, arr, R.FLOW_TCP, known=known)
    check_shape(len(frames), 4, od, oi, og, counts)
    assert list(counts) == [4 + 4, len(frames)]
    lists = groups_as_lists(oi, og, 8)
    got = recovered(perm, groups, range(6), lists)
    assert got[4] == 0 and got[1] == 2 and lists[1] == [] and lists[3] == []
    assert sorted(got[f] for f in (0, 2, 3, 5)) == [4, 5, 6, 7]


# ---------------------------------------------------------------- the gather batches' fixtures, interleaved

def test_reasm_ipv4_single_key_groups_are_recovered():
    """No (src, dst, id) is shared by two of the 300 groups and 280 of them hold one key; 250 of those are
    made of fragments and come back member for member.  The other 30 are single datagrams with neither MF
    nor an offset: the FRAG4 rule leaves them unselected (pico_ipv4_process_in does not hand them to the
    reassembly either)."""
    buf, arr, perm, groups, keys = reasm_batch("v4")
    off = fixture("ref_reasm_cases.npz")["v4_frag_off"]
    raw = lambda i: bytes(buf[int(off[i]) + 4:int(off[i]) + 6]) + bytes(buf[int(off[i]) + 12:int(off[i]) + 20])   # id, src, dst
    raw_single = [g for g, (f, c) in enumerate(groups) if len({raw(i) for i in range(f, f + c)}) == 1]
    assert len(raw_single) == 280
    owner = {}
    for g, (f, c) in enumerate(groups):
        for i in range(f, f + c):
            assert owner.setdefault(raw(i), g) == g
    single = single_key_groups(groups, keys)
    assert len(single) == 250 and set(single) <= set(raw_single)
    lone = sorted(set(raw_single) - set(single))
    assert len(lone) == 30 and all(groups[g][1] == 1 and keys[groups[g][0]] is None for g in lone)
    od, oi, og, counts = R.group(buf, arr, R.FLOW_FRAG4)
    check_shape(arr.shape[0], 0, od, oi, og, counts)
    assert int(counts[1]) == arr.shape[0] - 30
    got = recovered(perm, groups, single, groups_as_lists(oi, og, int(counts[0])))
    assert None not in got.values() and len(set(got.values())) == 250
    # the rest follow the key rule: every group holds one key, and no key is in two groups
    seen = set()
    for m in groups_as_lists(oi, og, int(counts[0])):
        ks = {keys[int(perm[i])] for i in m}
        assert len(ks) == 1 and not (ks & seen)
        seen |= ks


def test_reasm_ipv6_single_key_groups_are_recovered():
    """IPv6: 265 of the 300 groups are made of selected fragments of one key (counted here with the
    restatement; 26 more hold one key beside a fragment whose extension-header chain the walk discards)."""
    buf, arr, perm, groups, keys = reasm_batch("v6")
    single = single_key_groups(groups, keys)
    assert len(single) == 265
    od, oi, og, counts = R.group(buf, arr, R.FLOW_FRAG6)
    check_shape(arr.shape[0], 0, od, oi, og, counts)
    assert int(counts[1]) == sum(k is not None for k in keys)
    got = recovered(perm, groups, single, groups_as_lists(oi, og, int(counts[0])))
    assert None not in got.values() and len(set(got.values())) == 265


def test_tcprx_connections_are_recovered():
    a = fixture("ref_tcprx_cases.npz")
    desc = batch.make_desc(a["off"], a["len"])
    arr, perm = synth.interleave_groups(desc, a["group"], seed=23)
    od, oi, og, counts = R.group(a["buf"], arr, R.FLOW_TCP)
    check_shape(arr.shape[0], 0, od, oi, og, counts)
    assert list(counts) == [24, arr.shape[0]]
    got = recovered(perm, a["group"], range(24), groups_as_lists(oi, og, 24))
    assert None not in got.values() and len(set(got.values())) == 24


# ---------------------------------------------------------------- the key, pinned to pico_socket_tcp_deliver

def flowgroup_known(a) -> np.ndarray:
    return R.make_known([(4, bytes(a["src"][t]), bytes(a["dst"][t]), int(a["sport"][t]), int(a["dport"][t]))
                         for t in range(a["sport"].size)])


def test_reference_sockets_read_their_groups():
    """Grouping the interleaved burst with the 8 tuples as the table gives, per table index, exactly the
    segments whose payloads the reference's child socket read."""
    a = fixture("ref_flowgroup_cases.npz")
    n = a["off"].size
    desc = batch.make_desc(a["off"], a["len"])
    od, oi, og, counts = R.group(a["buf"], desc, R.FLOW_TCP, known=flowgroup_known(a))
    check_shape(n, 8, od, oi, og, counts)
    assert list(counts) == [8, n]                           # no group beside the table's
    ro = np.concatenate([[0], np.cumsum(a["read_len"].astype(np.int64))])
    for t, m in enumerate(groups_as_lists(oi, og, 8)):
        assert m == [int(i) for i in np.where(a["owner"] == t)[0]]
        pay = [a["buf"][int(a["off"][i]) + 20 + 4 * (int(a["buf"][int(a["off"][i]) + 32]) >> 4):int(a["off"][i]) + int(a["len"][i])]
               for i in m]
        np.testing.assert_array_equal(np.concatenate(pay), a["read"][ro[t]:ro[t + 1]], err_msg=f"socket {t}")
    assert ((a["rcv_after"].astype(np.int64) - a["rcv_before"]) & 0xFFFFFFFF == a["read_len"]).all()


def test_binding_constants_match_the_restatement():
    assert (_lib.FLOW_TCP, _lib.FLOW_FRAG4, _lib.FLOW_FRAG6, _lib.FLOW_F_ETH) == (R.FLOW_TCP, R.FLOW_FRAG4, R.FLOW_FRAG6, R.FLOW_F_ETH)
    assert batch.FLOW_KEY_DTYPE == R.FLOW_KEY_DTYPE
