"""GPU: a burst's ICMPv4 answers (pico_icmp4_reply_batch_dev) against the numpy restatement of its contract
(tests/icmp4_ref.py, pinned to the compiled reference stack by tests/test_ref_icmp4.py) and against that
stack's own answers (tests/golden/ref_icmp4_cases.npz).  Every case compares the verdicts, the answers'
descriptors, the carried state and the WHOLE output buffer, canary-filled around tight regions (a region
is exactly its answer's size unless a case says otherwise), byte for byte."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests import icmp4_ref as I
from tests import test_ref_icmp4 as RF
from tests.gpu_util import DEV, pairs_dev, replay_captured, to_dev

pytestmark = pytest.mark.gpu

CANARY = 0xA5
OK, MF, UT, DU = I.V_ACCEPT, I.V_MALFORMED, I.V_UNTOUCHED, I.V_DUPLICATE
NOSTATE = "none"


def dev_desc(d):
    return to_dev(d.view(np.uint8)) if d.size else torch.zeros(16, dtype=torch.uint8, device=DEV)


def run_arrays(buf, desc, req, od, osize, st=None, d_st=NOSTATE):
    """The batch on the device against the restatement, everything compared.  st: the restatement's state
    (updated) or None; d_st: the device's state tensor, NOSTATE = a fresh one when st is given, else NULL.
    Returns (verdicts, out_ans, the expected buffer) and the device tensors (out, out_ans, state)."""
    n = desc.size
    want = np.full(osize, CANARY, np.uint8)
    if d_st is NOSTATE:
        d_st = None if st is None else to_dev(st.view(np.uint8))
    wv, woa = I.reply_batch(buf, desc, req, st, want, od)
    out = torch.full((osize,), CANARY, dtype=torch.uint8, device=DEV)
    gv, goa = batch.icmp4_reply_batch(to_dev(buf), dev_desc(desc), n, to_dev(req.view(np.uint8)), out, dev_desc(od), state=d_st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(gv.cpu().numpy(), wv)
    got = goa.cpu().numpy().view(I.DESC_DTYPE)
    for k in ("off", "len", "seed"):
        np.testing.assert_array_equal(got[k], woa[k], err_msg=k)
    bad = np.flatnonzero(out.cpu().numpy() != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8].tolist()}"
    if st is not None:
        np.testing.assert_array_equal(d_st.cpu().numpy().view(I.STATE_DTYPE), st)
    return (wv, woa, want), (out, goa, d_st)


def run(dgrams, types, codes=0, st=None, d_st=NOSTATE, **kw):
    buf, off, ln, req, ooff, cap, osize = synth.icmp4_burst(dgrams, types, codes, **kw)
    return run_arrays(buf, batch.make_desc(off, ln), req, batch.make_desc(ooff, cap), osize, st, d_st)


def echo(rng, T, ident=None, seq=None, **kw):
    ident = int(rng.integers(1 << 16)) if ident is None else ident
    seq = int(rng.integers(1 << 16)) if seq is None else seq
    return synth.icmp4_echo_request(rng, T, ident, seq, **kw)


# ---------------------------------------------------------------- the reference's own answers

@pytest.mark.parametrize("out_off", [0, 5])
def test_reference_fixture(out_off):
    """The 20 datagrams the compiled reference stack took, in one batch: the kernel writes the answer the
    stack itself sent to each, byte for byte, and nothing where the stack sent nothing."""
    a = RF.fixture()
    buf, desc, req, od, osize = RF.batch_of(a)
    od = od.copy()
    od["off"] += out_off
    (wv, woa, want), _ = run_arrays(buf, desc, req, od, osize + 16, I.state())
    woa = woa.copy()
    woa["off"][woa["len"] > 0] -= out_off
    RF.check_against_reference(a, wv, woa, np.concatenate([want[out_off:], want[:out_off]]), f"out_off {out_off}", CANARY)


# ---------------------------------------------------------------- alignments, lengths, the read rule

def test_alignment_grid():
    """Request offset = 0, 1, 2, 15 mod 16 x region offset = 0, 1, 4, 15 mod 16 x T in {8, 9, 23, 24, 25, 40,
    41, 1480, 4097}, every combination in one batch of tight regions; DF set and clear, IHL 5 and 6."""
    rng = np.random.default_rng(1)
    combos = [(a, o, T) for a in (0, 1, 2, 15) for o in (0, 1, 4, 15) for T in (8, 9, 23, 24, 25, 40, 41, 1480, 4097)]
    dgrams = [echo(rng, T, ident=k, seq=k, frag=0x4000 * (k & 1), ihl=5 + (k % 3 == 0)) for k, (_, _, T) in enumerate(combos)]
    (wv, _, _), _ = run(dgrams, 0, align=[c[0] for c in combos], out_off=[c[1] for c in combos])
    assert (wv == OK).all()


@pytest.mark.parametrize("align,out_off", [(0, 0), (3, 9), (15, 4)])
def test_longest_answer(align, out_off):
    """65515 transport bytes: an answer of 65535 (documented difference 2: written whole)."""
    rng = np.random.default_rng(2)
    (wv, woa, _), _ = run([echo(rng, 65515)], 0, align=align, out_off=out_off)
    assert wv[0] == OK and woa["len"][0] == 65535


@pytest.mark.parametrize("tail", [0, 1, 15])
def test_last_block_read_rule(tail):
    """A request whose last byte is the last byte of the buffer, and one ending 1 and 15 bytes before it; T
    and the alignments chosen so that the mover's last unit straddles the end."""
    rng = np.random.default_rng(3)
    for T, align, out_off in ((8, 0, 0), (23, 5, 11), (24, 12, 3), (41, 1, 0), (1480, 7, 13), (64, 8, 8)):
        dgrams = [echo(rng, 19), echo(rng, T)]
        buf, off, ln, req, ooff, cap, osize = synth.icmp4_burst(dgrams, 0, align=[0, align], out_off=out_off)
        buf = np.concatenate([buf, synth.random_bytes(tail, tail)])
        assert int(off[1]) + int(ln[1]) + tail == buf.size
        (wv, _, _), _ = run_arrays(buf, batch.make_desc(off, ln), req, batch.make_desc(ooff, cap), osize)
        assert (wv == OK).all()


def test_trailer_is_not_copied():
    rng = np.random.default_rng(4)
    (wv, woa, _), _ = run([echo(rng, T) for T in (8, 13, 56)], 0, slack=[1, 7, 18], out_off=2)
    assert (wv == OK).all() and woa["len"].tolist() == [28, 33, 76]


# ---------------------------------------------------------------- pairs

@pytest.mark.parametrize("n", [1, 3, 5])
def test_odd_counts_and_lone_members(n):
    """An odd count leaves the last wave a lone member; records that write nothing leave their partner alone."""
    rng = np.random.default_rng(5)
    dgrams = [echo(rng, 9 + 31 * k, icmp_type=0 if k == 1 else 8) for k in range(n)]
    (wv, _, _), _ = run(dgrams, 0, align=3, out_off=7)
    assert wv.tolist() == [OK, UT, OK, OK, OK][:n]


@pytest.mark.parametrize("order", [(0, 11), (11, 0), (3, 12), (0, 0)])
def test_a_pair_of_one_echo_and_one_notice(order):
    rng = np.random.default_rng(6)
    (wv, woa, _), _ = run([echo(rng, 100), echo(rng, 77)], list(order), codes=[1, 3], align=[1, 2], out_off=[15, 6])
    assert (wv == OK).all() and woa["len"].tolist() == [120 if order[0] == 0 else 56, 97 if order[1] == 0 else 56]


def test_both_launch_shapes():
    """One batch on each side of the launch-shape threshold (datagrams averaging 1024 bytes: a wave takes two
    records below it, one from it on): the same records, the buffer one byte short of 1024 n and exactly
    1024 n long.  Both equal the restatement, so results do not depend on the shape."""
    rng = np.random.default_rng(15)
    dgrams = [echo(rng, T, ihl=5 + k % 2) for k, T in enumerate((8, 41, 300, 700, 65, 1480, 23))]
    types = [0, 11, 0, 0, 3, 0, 0]
    buf, off, ln, req, ooff, cap, osize = synth.icmp4_burst(dgrams, types, align=np.arange(7) * 5 % 16, out_off=np.arange(7) * 3 % 16)
    assert buf.size < 1024 * 7 - 1
    outs = []
    for size in (1024 * 7 - 1, 1024 * 7):
        b = np.concatenate([buf, synth.random_bytes(size, size - buf.size)])
        (wv, _, want), _ = run_arrays(b, batch.make_desc(off, ln), req, batch.make_desc(ooff, cap), osize)
        assert (wv == OK).all()
        outs.append(want)
    np.testing.assert_array_equal(outs[0], outs[1])


# ---------------------------------------------------------------- duplicates

def test_a_run_of_equal_requests():
    rng = np.random.default_rng(7)
    dgrams = [echo(rng, 8 + k, ident=0x1234, seq=9) for k in range(70)] + [echo(rng, 12, ident=0x1234, seq=10)]
    st = I.state()
    (wv, _, _), _ = run(dgrams, 0, st=st)
    assert wv.tolist() == [OK] + [DU] * 69 + [OK]
    assert (int(st["seen"][0]), int(st["id"][0]), int(st["seq"][0])) == (1, 0x3412, 0x0A00)


def test_equal_pairs_across_gaps():
    """Equal (id, seq) with 1, 63, 64, 255, 256 and 700 records that are no echo requests in between (notices,
    an echo reply coming in, a MALFORMED record): still duplicates -- the backward scan crosses wave and
    workgroup boundaries -- while one real request in between makes the repeat a fresh one."""
    rng = np.random.default_rng(8)
    dgrams, types = [], []
    for k, gap in enumerate((1, 63, 64, 255, 256, 700)):
        e = echo(rng, 10 + k, ident=0x100 + k, seq=k)
        dgrams.append(e)
        types.append(0)
        for j in range(gap):
            kind = j % 3
            dgrams.append(echo(rng, 8, icmp_type=0) if kind == 0 else echo(rng, 8)[:19 if kind == 2 else 28])
            types.append((0, 11, 3)[kind])
        dgrams.append(e.copy())
        types.append(0)
    p = echo(rng, 16, ident=7, seq=7)
    dgrams += [p, echo(rng, 16, ident=7, seq=8), p.copy()]
    types += [0, 0, 0]
    st = I.state()
    (wv, _, _), _ = run(dgrams, types, st=st, region=64)
    firsts = np.cumsum([0] + [g + 2 for g in (1, 63, 64, 255, 256, 700)])
    assert (wv[firsts[:-1]] == OK).all() and (wv[firsts[1:] - 1] == DU).all()
    assert wv[-3:].tolist() == [OK, OK, OK] and (wv == MF).sum() == sum(g // 3 for g in (1, 63, 64, 255, 256, 700))


def test_state_across_two_calls_and_none():
    rng = np.random.default_rng(9)
    p, q = echo(rng, 20, ident=5, seq=6), echo(rng, 21, ident=5, seq=7)
    st = I.state()
    (v1, _, _), (_, _, d_st) = run([q, p], 0, st=st)
    (v2, _, _), _ = run([p.copy(), q.copy()], 0, st=st, d_st=d_st)          # the same device state, carried
    assert v1.tolist() == [OK, OK] and v2.tolist() == [DU, OK]
    (v3, _, _), _ = run([echo(rng, 8, icmp_type=0)], [0], st=st, d_st=d_st)  # no echo request: the state stays
    assert v3.tolist() == [UT] and int(st["seen"][0]) == 1
    (v4, _, _), _ = run([q.copy(), q.copy()], 0, st=None)                    # d_state NULL: nothing carried, nothing kept
    assert v4.tolist() == [OK, DU]


# ---------------------------------------------------------------- verdicts

def test_malformed_and_untouched_write_nothing():
    rng = np.random.default_rng(10)
    good = lambda: echo(rng, 24)
    cases = []                                             # (datagram, type, desc.len delta, region delta, name)
    d = good(); d[0] = 0x65; cases.append((d, 0, 0, 0, "version"))
    d = good(); d[0] = 0x44; cases.append((d, 0, 0, 0, "IHL < 5"))
    d = good(); d[9] = 17; cases.append((d, 0, 0, 0, "proto"))
    d = good(); d[3] = 27; cases.append((d, 0, 0, 0, "len field < IHL 4 + 8"))
    cases.append((good(), 0, -1, 0, "len field > desc.len"))
    cases.append((good()[:19], 0, 0, 0, "fewer than 20 bytes"))
    cases.append((good(), 8, 0, 0, "req.type 8"))
    cases.append((good(), 5, 0, 0, "req.type 5"))
    cases.append((good(), 0, 0, -1, "region one byte short"))
    cases.append((good(), 11, 0, -1, "a notice's region one byte short"))
    d = good(); d[2], d[3] = 0, 19; cases.append((d, 3, 0, 0, "a notice's len field < 20"))
    cases.append((good()[:27], 12, 0, 0, "q > desc.len"))
    d = good(); d[20] = 0; cases.append((d, 0, 0, 0, "untouched: echo reply"))
    d = good(); d[20] = 3; cases.append((d, 0, 0, 0, "untouched: unreachable"))
    cases.append((good(), 0, 0, 0, "fine"))
    buf, off, ln, req, ooff, cap, osize = synth.icmp4_burst([c[0] for c in cases], [c[1] for c in cases], out_off=1,
                                                            slack=[c[2] for c in cases])
    cap = np.where(cap > 20, cap, 44).astype(np.int64) + np.array([c[3] for c in cases])
    ooff = np.concatenate([[0], np.cumsum(cap[:-1] + 3)]).astype(np.uint64) + 1
    osize = int(ooff[-1] + cap[-1] + 16)
    desc, od = batch.make_desc(off, ln), batch.make_desc(ooff, cap)
    # descriptors and regions past the buffers
    desc = np.concatenate([desc, batch.make_desc([buf.size + 1, buf.size - 10], [44, 44])])
    req = np.concatenate([req, req[-1:], req[-1:]])
    od = np.concatenate([od, od[-1:], od[-1:]])
    d2, o2, r2 = desc[-3:].copy(), od[-3:].copy(), req[-3:].copy()
    d2[:] = desc[len(cases) - 1]
    o2["off"], o2["len"] = [osize + 1, osize - 10, 2 ** 40], [44, 44, 44]
    (wv, woa, want), _ = run_arrays(buf, np.concatenate([desc, d2]), np.concatenate([req, r2]), np.concatenate([od, o2]), osize,
                                    I.state())
    names = [c[4] for c in cases]
    assert wv[:len(cases)].tolist() == [MF] * 12 + [UT, UT, OK], dict(zip(names, wv.tolist()))
    assert wv[len(cases):].tolist() == [MF] * 5
    assert (woa["len"][wv != OK] == 0).all() and (woa["off"][wv != OK] == 0).all()


def test_notices():
    """IHL 5, 6 and 15 (the quote holds option bytes), len field 20, 27, 28 and 29, types 3, 11, 12 with odd
    codes, at every region alignment mod 4 and a few request alignments."""
    rng = np.random.default_rng(11)
    dgrams, types, codes = [], [], []
    for k, (ihl, tot) in enumerate([(5, 20), (5, 27), (5, 28), (5, 29), (6, 32), (6, 24), (15, 68), (15, 60), (5, 1500), (5, 21)]):
        for typ in (3, 11, 12):
            d = echo(rng, max(tot - 4 * ihl, 8), ihl=ihl)[:max(tot, 20)].copy()
            d[2], d[3] = tot >> 8, tot & 0xFF
            if tot < 4 * ihl:
                d = np.concatenate([d, rng.integers(0, 256, 4 * ihl - tot, dtype=np.uint8)])   # (readable bytes behind the quote)
            dgrams.append(d)
            types.append(typ)
            codes.append((k * 7 + typ) & 0xFF)
    n = len(dgrams)
    (wv, woa, want), _ = run(dgrams, types, codes, align=np.arange(n) * 5 % 16, out_off=np.arange(n) * 3 % 16)
    assert (wv == OK).all()
    for i in range(n):
        tot = int(dgrams[i][2]) << 8 | int(dgrams[i][3])
        assert woa["len"][i] == 28 + min(tot, 28)
        a = want[int(woa["off"][i]):][:int(woa["len"][i])]
        assert O.checksum(a[:20]) == 0 and O.checksum(a[20:]) == 0 and bytes(a[24:28]) == b"\0\0\x05\xdc"


# ---------------------------------------------------------------- round trips

def test_answers_verify_in_the_rx_batch():
    """Answers <= MTU go through ipv4_checksum_batch RX as they lie: ACCEPT, both results 0."""
    rng = np.random.default_rng(12)
    dgrams = [echo(rng, T, ihl=5 + k % 2) for k, T in enumerate((8, 9, 64, 65, 777, 1479, 1480))] + [echo(rng, 40), echo(rng, 90)]
    (wv, _, _), (out, goa, _) = run(dgrams, [0] * 7 + [3, 11], codes=4, align=9, out_off=[0, 1, 2, 3, 4, 5, 6, 7, 15])
    assert (wv == OK).all()
    net, l4, v = batch.ipv4_checksum_batch(out, goa, len(dgrams))
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == batch.V_ACCEPT).all() and (net.cpu().numpy() == 0).all() and (l4.cpu().numpy() == 0).all()


def test_long_answers_through_fragmentation_and_reassembly():
    """One 9000-byte and one 65515-byte answer go through ipv4_fragment_batch unchanged (documented
    difference 2), then ipv4_reassemble_batch: ACCEPT, the bytes equal the answer (the header's len / frag /
    crc are the first fragment's own)."""
    rng = np.random.default_rng(13)
    dgrams = [echo(rng, 9000 - 20), echo(rng, 65515)]
    (wv, woa, want), (out, goa, _) = run(dgrams, 0, align=[3, 0], out_off=[6, 1])
    assert (wv == OK).all() and woa["len"].tolist() == [9000, 65535]
    cnt = (woa["len"].astype(np.int64) - 20 + 1479) // 1480
    groups = np.stack([np.concatenate([[0], np.cumsum(cnt[:-1])]), cnt], axis=1).astype(np.uint32)
    n_frag = int(cnt.sum())
    fo = 12 + np.concatenate([[0], np.cumsum(cnt[:-1] * 1504 + 16)])
    f_out = torch.zeros(int(fo[-1] + cnt[-1] * 1504 + 16), dtype=torch.uint8, device=DEV)
    d_of, d_grp = torch.zeros(16 * n_frag, dtype=torch.uint8, device=DEV), pairs_dev(groups)
    v, c, _ = batch.ipv4_fragment_batch(out, goa, 1500, d_grp, n_frag, f_out, dev_desc(batch.make_desc(fo, cnt * 1504)), 1504,
                                        out_frag=d_of)
    ro = np.array([12, 12 + 9008])
    r_out = torch.zeros(12 + 9008 + 65535 + 16, dtype=torch.uint8, device=DEV)
    ol, rl4, rv = batch.ipv4_reassemble_batch(f_out, d_of, n_frag, d_grp, r_out, dev_desc(batch.make_desc(ro, woa["len"])))
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == batch.V_ACCEPT).all() and c.cpu().numpy().tolist() == cnt.tolist()
    assert (rv.cpu().numpy() == batch.V_ACCEPT).all() and ol.cpu().numpy().tolist() == (woa["len"] - 20).tolist()
    got = r_out.cpu().numpy()
    for g in range(2):
        a = want[int(woa["off"][g]):][:int(woa["len"][g])].copy()
        have = got[int(ro[g]):][:a.size]
        a[[2, 3, 6, 7, 10, 11]] = have[[2, 3, 6, 7, 10, 11]]
        np.testing.assert_array_equal(have, a, err_msg=f"answer {g}")
        assert O.checksum(have[20:]) == 0


# ---------------------------------------------------------------- one graph

def test_forwarding_and_notices_in_one_graph():
    """pico_ipv4_forward_batch_dev + pico_icmp4_reply_batch_dev captured into one graph on one stream and
    replayed on two different bursts: every datagram carries a Time Exceeded record (the host sends the ones
    whose verdict is V_EXPIRED), quoted as the forwarding step left it -- the decremented ttl, the
    incremented crc -- plus two echo requests whose duplicate state is carried from replay to replay."""
    rng = np.random.default_rng(14)
    n = 40
    bursts = []
    for b in range(2):
        dgrams = [echo(rng, 8 + int(rng.integers(0, 60)), ident=3, seq=4, ihl=5 + k % 2) for k in range(n)]
        for k, d in enumerate(dgrams):
            d[8] = 1 if k % 3 else 9                        # ttl 1: expires
        types = [11] * n
        types[5] = types[17] = 0
        bursts.append(synth.icmp4_burst(dgrams, types, align=np.arange(n) % 16, out_off=np.arange(n) * 7 % 16, seed=20 + b))
    size = max(b[0].size for b in bursts)
    osize = max(b[6] for b in bursts)
    base = torch.zeros(size, dtype=torch.uint8, device=DEV)
    d_desc, d_req, d_od = (torch.zeros(16 * n, dtype=torch.uint8, device=DEV), torch.zeros(8 * n, dtype=torch.uint8, device=DEV),
                           torch.zeros(16 * n, dtype=torch.uint8, device=DEV))
    out = torch.full((osize,), CANARY, dtype=torch.uint8, device=DEV)
    fv = torch.zeros(n, dtype=torch.uint8, device=DEV)
    res = (torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(16 * n, dtype=torch.uint8, device=DEV))
    fst, ist = batch.fwd_state(DEV), batch.icmp4_state(DEV)
    h_fst, h_ist = O.fwd_state(), I.state()

    def load(b):
        buf, off, ln, req, ooff, cap, _ = bursts[b]
        base.zero_()
        base[:buf.size].copy_(to_dev(buf))
        d_desc.copy_(dev_desc(batch.make_desc(off, ln)))
        d_req.copy_(to_dev(req.view(np.uint8)))
        d_od.copy_(dev_desc(batch.make_desc(ooff, cap)))

    def call(s):
        batch.ipv4_forward_batch(base, d_desc, n, state=fst, verdict=fv, stream=s)
        batch.icmp4_reply_batch(base, d_desc, n, d_req, out, d_od, state=ist, stream=s, results=res)

    load(0)
    call(None)                                              # warm (eager)
    torch.cuda.synchronize()
    turn = [0]

    def reset():
        load(turn[0])
        out.fill_(CANARY)
        fst.zero_()
        if turn[0] == 0:
            ist.zero_()                                     # (the second replay carries the first one's echo state)
        for t in res + (fv,):
            t.zero_()
        torch.cuda.synchronize()                            # the replay starts from finished copies

    def check():
        buf, off, ln, req, ooff, cap, _ = bursts[turn[0]]
        b = np.zeros(size, np.uint8)
        b[:buf.size] = buf
        desc = batch.make_desc(off, ln)
        h_fst[:] = 0
        wf = O.batch_ipv4_forward(b, desc, state=h_fst)
        want = np.full(osize, CANARY, np.uint8)
        wv, woa = I.reply_batch(b, desc, req, h_ist, want, batch.make_desc(ooff, cap))
        np.testing.assert_array_equal(fv.cpu().numpy(), wf)
        assert (wf == batch.V_EXPIRED).sum() >= n // 2
        np.testing.assert_array_equal(res[0].cpu().numpy(), wv)
        np.testing.assert_array_equal(res[1].cpu().numpy().view(I.DESC_DTYPE)["len"], woa["len"])
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        np.testing.assert_array_equal(ist.cpu().numpy().view(I.STATE_DTYPE), h_ist)
        assert wv[[5, 17]].tolist() == ([OK, DU] if turn[0] == 0 else [DU, DU])
        turn[0] += 1

    replay_captured(call, reset, check, times=2)
