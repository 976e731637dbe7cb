"""GPU: the argument checks of picotcp_amd/batch.py's wrappers, one case per check, on a batch of 2
groups with 3 members each (a few hundred bytes: the smallest shape at which every check can go
wrong).  A rejected call must raise ValueError BEFORE the library is reached: every rejection case
replaces picotcp_amd._lib.load with a function that raises, so a lost check fails here and does not
send a short tensor to a kernel.  The valid calls (the real library) pin what the checks let through:
`results` / `out` left out, passed preallocated (the objects come back), every optional output None,
and the descriptors as int64 tensors -- the same outputs each time."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from picotcp_amd import _lib, batch, synth
from tests.gpu_util import DEV, pairs_dev, to_dev

pytestmark = pytest.mark.gpu

N, M = 2, 6                                            # groups, members (3 a group)
I16, I32, U8 = torch.int16, torch.int32, torch.uint8


def desc_dev(off, ln, seed=None):
    return to_dev(batch.make_desc(off, ln, seed).view(np.uint8))


def zeros(k):
    return torch.zeros(k, dtype=U8, device=DEV)


@functools.lru_cache(maxsize=None)
def _host(kind):
    """The numpy side of every valid call, built once."""
    if kind in ("reasm4", "reasm6"):
        f = synth.ipv4_fragments if kind == "reasm4" else synth.ipv6_fragments
        buf, off, flen, grp = f([40, 48], seed=5, proto=17 if kind == "reasm4" else 6, frag_payload=16)
        assert off.size == M
        return buf, off, flen, grp
    if kind == "fragment":
        r = synth.ipv4_oversized([40, 48], mtu=36, stride=40, seed=6)
        assert r[6] == M
        return r
    if kind == "segment":
        r = synth.tcp_streams([40, 48], per=16, stride=80, seed=7)
        assert r[7] == M
        return r
    if kind == "coalesce":
        rng, conns = np.random.default_rng(8), []
        for g, P in enumerate((40, 48)):
            data, rcv = synth.random_bytes(80 + g, P), 1000 * (g + 1)
            conns.append(([synth.tcp_rx_frame(rng, rcv + a, data[a:a + 16]) for a in range(0, P, 16)], rcv, False, P))
        return synth.tcp_rx_pack(conns)
    if kind == "v4":
        return synth.ipv4_batch([60, 72], seed=9)
    if kind == "v6":
        return synth.ipv6_batch([80, 92], seed=10)
    if kind == "eth":
        return synth.eth_batch(N, seed=11)
    raise KeyError(kind)


def reasm_args(kind):
    buf, off, flen, grp = _host(kind)
    return dict(base=to_dev(buf), frag_desc=desc_dev(off, flen), n_frag=M, groups=pairs_dev(grp), out=zeros(288),
                out_desc=desc_dev([12, 156], [120, 120]))


def fragment_args():
    buf, off, dlen, groups, ooff, cap, n_frag, out_size = _host("fragment")
    return dict(base=to_dev(buf), dgram_desc=desc_dev(off, dlen), mtu=36, groups=pairs_dev(groups), n_frag=M,
                out=zeros(out_size), out_desc=desc_dev(ooff, cap), frag_stride=40, flags=batch.F_WRITE, out_frag=zeros(16 * M))


def segment_args():
    buf, off, slen, per, groups, ooff, cap, n_seg, out_size = _host("segment")
    return dict(base=to_dev(buf), stream_desc=desc_dev(off, slen, per), groups=pairs_dev(groups), n_seg=M,
                out=zeros(out_size), out_desc=desc_dev(ooff, cap), seg_stride=80, out_seg=zeros(16 * M))


def coalesce_args():
    buf, off, ln, groups, conn, ooff, cap, out_size = _host("coalesce")
    assert off.size == M
    return dict(base=to_dev(buf), seg_desc=desc_dev(off, ln), n_seg=M, groups=pairs_dev(groups), conn=pairs_dev(conn),
                out=zeros(out_size), out_desc=desc_dev(ooff, cap))


def rx_args(kind):
    buf, off, ln, *rest = _host(kind)
    return dict(base=to_dev(buf), desc=desc_dev(off, ln, rest[0] if rest else None), n=N)


def nat_args():
    kw = rx_args("v4")
    kw["nat"] = zeros(8 * N)                           # dir NAT_NONE: untouched
    return kw


TRIPLE = ((I16, N), (I16, N), (U8, N))
# per wrapper: the function, its valid keyword arguments, the tensor arguments, the descriptor arguments with
# their counts, the pair arguments after `groups`, the optional descriptor output, the name of the results
# argument with its members' (dtype, count), whether a member may be None, and where the verdicts come back
SPECS = {
    "ipv4_reassemble_batch": (batch.ipv4_reassemble_batch, functools.partial(reasm_args, "reasm4"),
                              ("base", "frag_desc", "groups", "out", "out_desc"), {"frag_desc": M, "out_desc": N}, (), None,
                              "results", ((I32, N), (I16, N), (U8, N)), False, 2),
    "ipv6_reassemble_batch": (batch.ipv6_reassemble_batch, functools.partial(reasm_args, "reasm6"),
                              ("base", "frag_desc", "groups", "out", "out_desc"), {"frag_desc": M, "out_desc": N}, (), None,
                              "results", ((I32, N), (I16, N), (U8, N)), False, 2),
    "ipv4_fragment_batch": (batch.ipv4_fragment_batch, fragment_args,
                            ("base", "dgram_desc", "groups", "out", "out_desc"), {"dgram_desc": N, "out_desc": N}, (), "out_frag",
                            "results", ((U8, N), (I32, N), (I16, N)), True, 0),
    "tcp_segment_batch": (batch.tcp_segment_batch, segment_args,
                          ("base", "stream_desc", "groups", "out", "out_desc"), {"stream_desc": N, "out_desc": N}, (), "out_seg",
                          "results", ((U8, N), (I32, N)), True, 0),
    "tcp_coalesce_batch": (batch.tcp_coalesce_batch, coalesce_args,
                           ("base", "seg_desc", "groups", "conn", "out", "out_desc"), {"seg_desc": M, "out_desc": N}, ("conn",),
                           None, "results", ((U8, N), (I32, N), (U8, M)), True, 0),
    # the older wrappers: the `out=` triple / pair, and the descriptor count
    "ipv4_checksum_batch": (batch.ipv4_checksum_batch, functools.partial(rx_args, "v4"), ("base", "desc"), {"desc": N}, (), None,
                            "out", TRIPLE, False, None),
    "ipv6_checksum_batch": (batch.ipv6_checksum_batch, functools.partial(rx_args, "v6"), ("base", "desc"), {"desc": N}, (), None,
                            "out", TRIPLE[1:], False, None),
    "eth_checksum_batch": (batch.eth_checksum_batch, functools.partial(rx_args, "eth"), ("base", "desc"), {"desc": N}, (), None,
                           "out", TRIPLE, False, None),
    "ipv4_nat_batch": (batch.ipv4_nat_batch, nat_args, ("base", "desc", "nat"), {"desc": N}, (), None,
                       "out", TRIPLE, False, None),
}


def members(spec, fill=None):
    return tuple(torch.empty(k, dtype=dt, device=DEV) if fill is None else torch.full((k,), fill, dtype=dt, device=DEV)
                 for dt, k in spec)


# the faults: each takes the valid tensor and returns the one a check must refuse
def cpu(t):
    return t.cpu()


def other_device(t):
    return t.to("cuda:1")


def not_u8(t):
    return t.to(I16)


def strided(t):
    return t.repeat_interleave(2)[::2]                 # the same elements, two apart


def eight_byte(t):
    return t.to(torch.int64)


def one_short(t):
    return t[:-1]                                      # (a descriptor tensor: one byte short of 16 * count)


def one_short_int64(t):
    return t.view(torch.int64)[:-1]                    # (the nearest an int64 tensor comes to it: 8 bytes short)


def wrong_item_size(t):
    return t.to(I32 if t.element_size() == 2 else I16)


def _cases():
    for w, (_, _, tensors, descs, pairs, opt, res_key, res_spec, _, _) in SPECS.items():
        new = res_key == "results"

        def arg(name, fault):
            return pytest.param(w, name, None, fault, id=f"{w}-{name}-{fault.__name__}")

        for nm in tensors:
            yield arg(nm, cpu)
            if new:                                    # (the older wrappers compare only their outputs' device)
                yield arg(nm, other_device)
        if new:
            for nm in ("base", "out"):
                yield arg(nm, not_u8)
                yield arg(nm, strided)
            for nm in ("groups",) + pairs:
                yield arg(nm, eight_byte)
                yield arg(nm, strided)
            for nm in pairs:
                yield arg(nm, one_short)
        for nm in descs:
            yield arg(nm, one_short)
            if new:
                yield arg(nm, one_short_int64)
        if opt:
            for fault in (one_short, one_short_int64, strided, cpu, other_device):
                yield arg(opt, fault)
        for i in range(len(res_spec)):
            for fault in (wrong_item_size, one_short, strided, cpu, other_device):
                yield pytest.param(w, res_key, i, fault, id=f"{w}-{res_key}{i}-{fault.__name__}")


def _no_launch():
    raise AssertionError("reached the launch")


@pytest.mark.parametrize("wrapper,name,member,fault", list(_cases()))
def test_rejected_before_the_launch(wrapper, name, member, fault, monkeypatch):
    fn, make, *_, res_key, res_spec, _, _ = SPECS[wrapper]
    if fault is other_device and torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    kw = make()
    if member is None:
        kw[name] = fault(kw[name])
    else:
        res = list(members(res_spec))
        res[member] = fault(res[member])
        kw[res_key] = tuple(res)
    monkeypatch.setattr(_lib, "load", _no_launch)
    with pytest.raises(ValueError):
        fn(**kw)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize("wrapper", list(SPECS))
def test_valid_calls_agree(wrapper):
    fn, make, _, descs, _, opt, res_key, res_spec, optional, verdict_at = SPECS[wrapper]

    def run(**over):
        kw = make()
        kw.update(over)
        res = fn(**kw)
        torch.cuda.synchronize()
        return res, [kw[k] for k in (("out", opt) if res_key == "results" else ()) if kw.get(k) is not None]

    r0, o0 = run()
    assert [(t.dtype, t.numel()) for t in r0] == list(res_spec)
    if verdict_at is not None:
        assert (r0[verdict_at] == batch.V_ACCEPT).all()
    pre = members(res_spec, fill=77)
    r1, o1 = run(**{res_key: pre})
    assert len(r1) == len(pre) and all(a is b for a, b in zip(r1, pre))
    _same(r1, r0)
    _same(o1, o0)
    if optional:
        over = {res_key: (None,) * len(res_spec)}
        if opt:
            over[opt] = None
        r2, o2 = run(**over)
        assert tuple(r2) == (None,) * len(res_spec)
        _same(o2, o0[:1])
    if res_key == "results":                           # the descriptors as int64 tensors, 2 elements each
        r3, o3 = run(**{d: make()[d].view(torch.int64) for d in descs})
        _same(r3, r0)
        _same(o3, o0)
