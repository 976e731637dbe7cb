"""The restatement of pico_icmp6_reply_batch_dev's contract (tests/icmp6_ref.py) pinned to the compiled
reference stack: tests/golden/ref_icmp6_cases.npz (tests/golden/make_ref_icmp6.py) holds 22 datagrams taken
through one stack in order, with the answer the stack itself sent to each -- or none.  Here (no GPU): the
restatement reproduces every answer byte for byte and writes nothing where the stack sent nothing;
tests/test_gpu_icmp6.py checks the kernel against the restatement and against this fixture.  Every row of
the fixture was captured (the echo to ff02::1 and the Time Exceeded included).  Pinned by the restatement
alone: Packet Too Big (type 2), which the reference never sends.  The three documented differences / rules
each have a named case: the trailer, type 2, repeats answered."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from picotcp_amd import batch, synth
from tests import icmp6_ref as I

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGION = 2048
TRAILER = 7                                                     # bytes behind the datagram of "echo with a trailer"
_fixture = None


def fixture():
    """The fixture's arrays (loaded once, shared, read-only)."""
    global _fixture
    if _fixture is None:
        c = np.load(os.path.join(GOLDEN, "ref_icmp6_cases.npz"))
        _fixture = {k: c[k] for k in c.files}
        for a in _fixture.values():
            a.setflags(write=False)
    return _fixture


def generator():
    sys.path.insert(0, GOLDEN)
    try:
        import make_ref_icmp6 as M
    finally:
        sys.path.remove(GOLDEN)
    return M


def batch_of(a):
    """The fixture as the batch's arguments: (buf, DESC, req, out DESC, out size)."""
    n = a["len"].size
    return a["buf"], batch.make_desc(a["off"], a["len"]), a["req"], batch.make_desc(np.arange(n) * REGION, np.full(n, REGION)), n * REGION


def reference_answers(a):
    o = np.concatenate([[0], np.cumsum(a["ans_len"].astype(np.int64))])
    return [bytes(a["ans"][o[i]:o[i + 1]]) for i in range(a["ans_len"].size)]


def check_against_reference(a, v, oa, out, note="", fill=0xEE):
    """Answers (of the restatement or of the kernel) against the reference stack's own, in full; `out` was
    filled with `fill`.  Every written answer's ICMPv6 checksum over its pseudo header sums to zero."""
    M = generator()
    for i, want in enumerate(reference_answers(a)):
        name = f"{a['name'][i]} {note}"
        got_len = int(oa["len"][i])
        if want:
            assert v[i] == I.V_ACCEPT, name
            got = bytes(out[REGION * i:REGION * i + got_len])
            assert M.valid_crc(got), name
            if a["differs"][i]:                                     # the trailer: the batch stops at the datagram's end
                assert got_len == len(want) - TRAILER and got[44:] == want[44:-TRAILER] and got[6:42] == want[6:42], name
            else:
                assert (int(oa["off"][i]), got_len, int(oa["seed"][i])) == (REGION * i, len(want), 0), name
                assert got == want, name
        else:
            assert v[i] == I.V_UNTOUCHED, name
            assert (int(oa["off"][i]), got_len, int(oa["seed"][i])) == (0, 0, 0), name
        assert (out[REGION * i + got_len:REGION * (i + 1)] == fill).all(), name       # nothing behind an answer, nothing without one


def restated(a):
    buf, desc, req, od, osize = batch_of(a)
    out = np.full(osize, 0xEE, np.uint8)
    v, oa = I.reply_batch(buf, desc, req, out, od)
    return v, oa, out


def one(d, typ=0, code=0, arg=0, hop=64, slack=0):
    """The restatement on one datagram: (verdict, answer bytes or None)."""
    req = np.zeros(1, I.REQ_DTYPE)
    req["src"], req["type"], req["code"], req["arg"], req["hop"] = np.arange(16) + 0x20, typ, code, arg, hop
    return I.answer(bytes(d) + b"\x55" * slack, req[0])


def test_restatement_reproduces_every_reference_answer():
    a = fixture()
    v, oa, out = restated(a)
    check_against_reference(a, v, oa, out)


def test_fixture_covers_the_cases():
    a = fixture()
    name = [str(x) for x in a["name"]]
    ans = dict(zip(name, reference_answers(a)))
    assert {len(x) - 40 for n, x in ans.items() if n.startswith("echo T=")} == {8, 9, 10, 11, 64, 65, 1232, 1233, 1460}
    assert not ans["echo reply coming in"] and not ans["unreachable coming in"]
    notices = {(x[40], x[41]) for x in ans.values() if x and x[40] != 129}
    assert notices == {(1, 4), (4, 1), (1, 3), (3, 0)}
    assert len(ans["UDP to a closed port, 1400 bytes"]) == 1280             # the quote capped at 1232
    assert ans["next header 200"][44:48] == b"\0\0\0\x06"
    assert ans["echo to ff02::1"][8:24] == bytes(a["req"]["src"][name.index("echo to ff02::1")])
    assert len(ans["echo behind hop-by-hop PadN"]) == 64                    # the extension header does not come back
    for x in ans.values():
        if x:
            assert x[:4] == b"\x60\0\0\0" and x[6] == 58


def test_generator_assertions_hold():
    generator().check(fixture())


def test_difference_the_trailer_is_not_echoed():
    """Documented difference 1: the reference echoes bytes behind the datagram (captured: 7 more bytes), the
    batch stops at the datagram's end."""
    a = fixture()
    i = [str(x) for x in a["name"]].index("echo with a trailer")
    assert a["differs"][i] == 1
    v, oa, _ = restated(a)
    assert v[i] == I.V_ACCEPT and int(oa["len"][i]) == 40 + 16 == int(a["ans_len"][i]) - TRAILER
    rng = np.random.default_rng(3)
    d = synth.icmp6_echo_request(rng, 13)
    (v0, a0), (v1, a1) = one(d), one(d, slack=9)
    assert v0 == v1 == I.V_ACCEPT and a0 == a1 and len(a0) == 53


def test_difference_packet_too_big():
    """Documented difference 2: type 2 has the notices' layout, the MTU in the word, code 0 forced and type 1's
    multicast rule; the reference sends nothing (pico_icmp6_notify's switch)."""
    M = generator()
    rng = np.random.default_rng(4)
    d = synth.udp6_datagram(rng, 1500)
    v, a = one(d, typ=2, code=9, arg=1280, hop=255)
    assert v == I.V_ACCEPT and len(a) == 1280 and a[40:42] == b"\x02\x00" and a[44:48] == (1280).to_bytes(4, "big")
    assert a[48:] == bytes(d[:1232]) and a[7] == 255 and a[24:40] == bytes(d[8:24]) and M.valid_crc(a)
    d[24] = 0xFF
    assert one(d, typ=2, arg=1280) == (I.V_UNTOUCHED, None)


def test_rule_repeats_are_answered():
    """No state: the same (id, seq) is answered every time, as the captured stack did."""
    a = fixture()
    name = [str(x) for x in a["name"]]
    v, oa, out = restated(a)
    i, j = name.index("echo P"), name.index("repeat of P")
    assert v[i] == v[j] == I.V_ACCEPT and a["ans_len"][i] == a["ans_len"][j] > 0
    assert bytes(out[REGION * i:][:73]) == bytes(out[REGION * j:][:73])


def test_restated_rules_beyond_the_fixture():
    M = generator()
    rng = np.random.default_rng(5)
    # notices: the multicast rule, the word, the quote's cap, q > desc.len
    d = synth.udp6_datagram(rng, 40)
    for typ in (1, 3):
        v, a = one(d, typ=typ, code=5, arg=77)
        assert v == I.V_ACCEPT and a[40:42] == bytes([typ, 5]) and a[44:48] == b"\0\0\0\0" and a[48:] == bytes(d) and M.valid_crc(a)
    m = d.copy()
    m[24] = 0xFF
    assert one(m, typ=1)[0] == one(m, typ=3)[0] == I.V_UNTOUCHED
    v, a = one(m, typ=4, code=2, arg=0x01020304)
    assert v == I.V_ACCEPT and a[44:48] == b"\x01\x02\x03\x04"                # type 4 is sent regardless
    assert one(d[:87], typ=1)[0] == I.V_MALFORMED                              # q > desc.len
    big = synth.udp6_datagram(rng, 2000)
    assert one(big[:1232], typ=1)[0] == I.V_ACCEPT and one(big[:1231], typ=1)[0] == I.V_MALFORMED
    # echo: the parse
    e = synth.icmp6_echo_request(rng, 24, 1, 2)
    assert one(e[:63])[0] == I.V_MALFORMED                                     # 40 + len field > desc.len
    x = e.copy(); x[0] = 0x40
    assert one(x)[0] == I.V_MALFORMED
    x = e.copy(); x[6] = 44
    assert one(x)[0] == I.V_UNTOUCHED                                          # a fragment
    x = e.copy(); x[6] = 17
    assert one(x)[0] == I.V_UNTOUCHED
    x = e.copy(); x[40] = 135
    assert one(x)[0] == I.V_UNTOUCHED                                          # a neighbour solicitation
    x = e[:47].copy(); x[5] = 7
    x = np.concatenate([x, np.zeros(20, np.uint8)])
    assert one(x)[0] == I.V_MALFORMED                                          # fewer than 8 transport bytes
    assert one(e[:39])[0] == I.V_MALFORMED and one(e, typ=5)[0] == I.V_MALFORMED
    h = synth.icmp6_echo_request(rng, 32, 1, 2, hbh=True)
    v, a = one(h)
    assert v == I.V_ACCEPT and len(a) == 72 and a[48:] == bytes(h[56:]) and a[8:24] == bytes(h[24:40]) and M.valid_crc(a)
    req = np.zeros(1, I.REQ_DTYPE)
    req["rsvd"] = 1
    assert I.answer(bytes(e), req[0])[0] == I.V_MALFORMED


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "libref_rx.so")),
                    reason="the reference stack is not compiled here")
def test_restatement_against_a_fresh_capture():
    """Another seed's traffic through a fresh compiled stack: the restatement gives the same answers."""
    M = generator()
    a = M.arrays(M.capture(seed=31))
    M.check(a)
    v, oa, out = restated(a)
    check_against_reference(a, v, oa, out, "(fresh capture)")
