"""The restatement of pico_icmp4_reply_batch_dev's contract (tests/icmp4_ref.py) pinned to the compiled
reference stack: tests/golden/ref_icmp4_cases.npz (tests/golden/make_ref_icmp4.py) holds 20 datagrams
taken through one stack in order, with the answer the stack itself sent to each -- or none.  Here (no
GPU): the restatement reproduces every answer byte for byte and writes nothing where the stack sent
nothing; tests/test_gpu_icmp4.py checks the kernel against the restatement and against this fixture.
Pinned by the restatement alone (the frozen driver's stack does not get there): requests with IPv4
options, answers above the MTU, and the notices 3 / 4, 3 / 13, 11 / 1 and 12 / x."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests import icmp4_ref as I

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGION = 2048
_fixture = None


def fixture():
    """The fixture's arrays (loaded once, shared, read-only)."""
    global _fixture
    if _fixture is None:
        c = np.load(os.path.join(GOLDEN, "ref_icmp4_cases.npz"))
        _fixture = {k: c[k] for k in c.files}
        for a in _fixture.values():
            a.setflags(write=False)
    return _fixture


def batch_of(a):
    """The fixture as the batch's arguments: (buf, DESC, req, out DESC, out size)."""
    n = a["len"].size
    return a["buf"], batch.make_desc(a["off"], a["len"]), a["req"], batch.make_desc(np.arange(n) * REGION, np.full(n, REGION)), n * REGION


def reference_answers(a):
    o = np.concatenate([[0], np.cumsum(a["ans_len"].astype(np.int64))])
    return [bytes(a["ans"][o[i]:o[i + 1]]) for i in range(a["ans_len"].size)]


def check_against_reference(a, v, oa, out, note="", fill=0xEE):
    """Answers (of the restatement or of the kernel) against the reference stack's own, in full; `out` was
    filled with `fill`."""
    for i, want in enumerate(reference_answers(a)):
        name = f"{a['name'][i]} {note}"
        if want:
            assert v[i] == I.V_ACCEPT, name
            assert (int(oa["off"][i]), int(oa["len"][i]), int(oa["seed"][i])) == (REGION * i, len(want), 0), name
            assert bytes(out[REGION * i:REGION * i + len(want)]) == want, name
        else:
            assert v[i] in (I.V_DUPLICATE, I.V_UNTOUCHED), name
            assert (int(oa["off"][i]), int(oa["len"][i]), int(oa["seed"][i])) == (0, 0, 0), name
        assert (out[REGION * i + len(want):REGION * (i + 1)] == fill).all(), name      # nothing behind an answer, nothing without one


def restated(a, st=None):
    buf, desc, req, od, osize = batch_of(a)
    out = np.full(osize, 0xEE, np.uint8)
    v, oa = I.reply_batch(buf, desc, req, I.state() if st is None else st, out, od)
    return v, oa, out


def test_restatement_reproduces_every_reference_answer():
    a = fixture()
    v, oa, out = restated(a)
    check_against_reference(a, v, oa, out)


def test_fixture_covers_the_cases():
    a = fixture()
    name = [str(x) for x in a["name"]]
    v, _, _ = restated(a)
    ans = reference_answers(a)
    T = {len(x) - 20 for n, x in zip(name, ans) if n.startswith("echo T=")}
    assert T == {8, 9, 10, 11, 64, 65, 1479, 1480}
    frag = {bytes(x[6:8]) for n, x in zip(name, ans) if n.startswith("echo T=")}
    assert frag == {b"\x40\x00", b"\x00\x00"}                       # DF set and clear come back as they came
    by = dict(zip(name, v.tolist()))
    assert by["repeat of P, same source"] == by["repeat of P, another source"] == I.V_DUPLICATE
    assert by["repeat of P behind Q"] == by["echo Q"] == I.V_ACCEPT
    assert by["echo reply coming in"] == by["unreachable coming in"] == I.V_UNTOUCHED
    # a corrupted request, a valid reply
    i = name.index("echo, wrong ICMP checksum")
    rq = a["buf"][int(a["off"][i]):int(a["off"][i]) + int(a["len"][i])]
    assert O.checksum(rq[20:]) != 0 and O.checksum(np.frombuffer(ans[i][20:], np.uint8)) == 0
    notices = {(x[20], x[21]) for n, x in zip(name, ans) if x and x[20] != 0}
    assert notices == {(3, 3), (3, 2), (11, 0), (3, 1)}
    for x in ans:
        if x:                                                       # tos 0, ttl 64, both checksums valid
            assert x[1] == 0 and x[8] == 64 and O.checksum(np.frombuffer(x[:20], np.uint8)) == 0
            assert O.checksum(np.frombuffer(x[20:], np.uint8)) == 0
    i = name.index("routed on with ttl 1")
    assert ans[i][28 + 8] == 0                                      # quoted as it lies: the decremented ttl


def test_generator_assertions_hold():
    sys.path.insert(0, GOLDEN)
    try:
        import make_ref_icmp4 as M
    finally:
        sys.path.remove(GOLDEN)
    M.check(fixture())


def test_state_is_carried_and_kept():
    a = fixture()
    buf, desc, req, od, osize = batch_of(a)
    name = [str(x) for x in a["name"]]
    k = name.index("repeat of P, same source")
    st = I.state()
    whole, _, _ = restated(a)
    out = np.full(osize, 0xEE, np.uint8)
    v1, _ = I.reply_batch(buf, desc[:k], req[:k], st, out, od[:k])
    assert int(st["seen"][0]) == 1 and (int(st["id"][0]), int(st["seq"][0])) == (0x0003, 0x0700)     # as stored: 03 00, 00 07
    v2, _ = I.reply_batch(buf, desc[k:], req[k:], st, out, od[k:])
    assert np.array_equal(np.concatenate([v1, v2]), whole)
    v3, _ = I.reply_batch(buf, desc[k:], req[k:], None, out, od[k:])      # nothing carried: the repeat is answered
    assert v3[0] == I.V_ACCEPT


def test_restated_rules_beyond_the_fixture():
    """What the frozen driver's stack does not produce, as the contract states it."""
    rng = np.random.default_rng(5)
    req = np.zeros(1, I.REQ_DTYPE)
    req["src"], req["id"] = 0x0100000A, 0x1234
    # documented difference 1: options are not copied, the answer has a 20-byte header
    d = synth.icmp4_echo_request(rng, 40, 7, 9, ihl=7)
    v, a, _ = I.answer(bytes(d), req[0])
    assert v == I.V_ACCEPT and len(a) == 60 and a[0] == 0x45 and a[28:] == bytes(d[36:]) and a[24:28] == bytes(d[32:36])
    assert O.checksum(np.frombuffer(a[20:], np.uint8)) == 0
    # documented difference 2: an answer above the MTU is written whole
    d = synth.icmp4_echo_request(rng, 65515)
    v, a, _ = I.answer(bytes(d), req[0])
    assert v == I.V_ACCEPT and len(a) == 65535 and a[2:4] == b"\xff\xff"
    # bytes behind the datagram are not copied
    d = synth.icmp4_echo_request(rng, 13)
    v, a, _ = I.answer(bytes(d) + b"\x55" * 9, req[0])
    assert len(a) == 33
    # notices: min(len field, 28) bytes whatever the IHL
    for typ, code in ((3, 4), (3, 13), (11, 1), (12, 0)):
        req["type"], req["code"] = typ, code
        for ihl, T in ((5, 0), (5, 7), (5, 8), (5, 9), (6, 20), (15, 8)):
            d = synth.icmp4_echo_request(rng, max(T, 8), ihl=ihl)
            if T < 8:
                d = d[:4 * ihl + T].copy()
                d[2], d[3] = 0, d.size
            v, a, _ = I.answer(bytes(d), req[0])
            q = min(d.size, 28)
            assert v == I.V_ACCEPT and len(a) == 28 + q and a[20:22] == bytes([typ, code]) and a[24:28] == b"\0\0\x05\xdc"
            assert a[28:] == bytes(d[:q]) and a[6:8] == b"\0\0" and O.checksum(np.frombuffer(a[20:], np.uint8)) == 0
    d = synth.icmp4_echo_request(rng, 8)
    assert I.answer(bytes(d[:27]), req[0])[0] == I.V_MALFORMED        # q > desc.len
    d[2], d[3] = 0, 19
    assert I.answer(bytes(d), req[0])[0] == I.V_MALFORMED             # len field < 20
    req["type"] = 5
    assert I.answer(bytes(d), req[0])[0] == I.V_MALFORMED


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "libref_rx.so")),
                    reason="the reference stack is not compiled here")
def test_restatement_against_a_fresh_capture():
    """Another seed's traffic through a fresh compiled stack: the restatement gives the same answers."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_ref_icmp4 as M
    finally:
        sys.path.remove(GOLDEN)
    a = M.arrays(M.capture(seed=29))
    M.check(a)
    v, oa, out = restated(a)
    check_against_reference(a, v, oa, out, "(fresh capture)")
