"""GPU: the argument checks of picotcp_amd.batch.tcp_ack_batch, one case per check, as
tests/test_gpu_batch_args.py has them for the other wrappers (its faults and its rule: a rejected call
raises ValueError BEFORE the library is reached), on the same batch of 2 connections with 3 segments
each.  The valid calls pin what the checks let through."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from picotcp_amd import _lib, batch, synth
from tests import test_gpu_batch_args as BA
from tests.gpu_util import DEV, pairs_dev, to_dev

pytestmark = pytest.mark.gpu

N, M = BA.N, BA.M
U8, I32 = torch.uint8, torch.int32


@functools.lru_cache(maxsize=None)
def _host():
    rng, conns = np.random.default_rng(8), []
    for g, P in enumerate((40, 48)):
        data, rcv = synth.random_bytes(80 + g, P), 1000 * (g + 1)
        frames = [synth.tcp_rx_frame(rng, rcv + a, data[a:a + 16]) for a in range(0, P, 16)]
        conns.append(([frames[0], frames[2], frames[0]], rcv, True, P))          # delivered, held, old
    return synth.tcp_rx_pack(conns), synth.tcp_ack_inputs(conns, ts_ok=1)


def ack_args():
    (buf, off, ln, groups, conn, ooff, cap, out_size), (tb, toff, tln, ak, foff, fcap, fsize) = _host()
    assert off.size == M
    base, seg, grp, cn = to_dev(buf), BA.desc_dev(off, ln), pairs_dev(groups), pairs_dev(conn)
    v, ol, sv = batch.tcp_coalesce_batch(base, seg, M, grp, cn, BA.zeros(out_size), BA.desc_dev(ooff, cap))
    return dict(base=base, seg_desc=seg, n_seg=M, groups=grp, conn=cn, out_len=ol, seg_verdict=sv, tmpl_base=to_dev(tb),
                tmpl_desc=BA.desc_dev(toff, tln), ack=to_dev(ak.view(np.uint8)), out=BA.zeros(fsize), out_desc=BA.desc_dev(foff, fcap))


TENSORS = ("base", "seg_desc", "groups", "conn", "out_len", "seg_verdict", "tmpl_base", "tmpl_desc", "ack", "out", "out_desc")
RES = ((U8, N), (U8, 16 * N))


def _cases():
    def arg(name, fault):
        return pytest.param(name, None, fault, id=f"{name}-{fault.__name__}")

    for nm in TENSORS:
        yield arg(nm, BA.cpu)
        yield arg(nm, BA.other_device)
    for nm in ("base", "tmpl_base", "out"):
        yield arg(nm, BA.not_u8)
        yield arg(nm, BA.strided)
    for nm in ("groups", "conn"):
        yield arg(nm, BA.eight_byte)
        yield arg(nm, BA.strided)
    yield arg("conn", BA.one_short)
    for nm in ("seg_desc", "tmpl_desc", "out_desc", "ack"):
        yield arg(nm, BA.one_short)
        yield arg(nm, BA.one_short_int64)
    yield arg("ack", BA.strided)
    for nm in ("out_len", "seg_verdict"):
        for fault in (BA.wrong_item_size, BA.one_short, BA.strided):
            yield arg(nm, fault)
    for i in range(len(RES)):
        for fault in (BA.wrong_item_size, BA.one_short, BA.strided, BA.cpu, BA.other_device):
            yield pytest.param("results", i, fault, id=f"results{i}-{fault.__name__}")


@pytest.mark.parametrize("name,member,fault", list(_cases()))
def test_rejected_before_the_launch(name, member, fault, monkeypatch):
    if fault is BA.other_device and torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    kw = ack_args()
    if member is None:
        kw[name] = fault(kw[name])
    else:
        res = list(BA.members(RES))
        res[member] = fault(res[member])
        kw["results"] = tuple(res)
    monkeypatch.setattr(_lib, "load", BA._no_launch)
    with pytest.raises(ValueError):
        batch.tcp_ack_batch(**kw)


def test_valid_calls_agree():
    def run(**over):
        kw = ack_args()
        kw.update(over)
        res = batch.tcp_ack_batch(**kw)
        torch.cuda.synchronize()
        return res, [kw["out"], kw["seg_verdict"]]

    r0, o0 = run()
    assert [(t.dtype, t.numel()) for t in r0] == list(RES)
    assert (r0[0] == batch.V_ACCEPT).all() and (r0[1].cpu().numpy().view(batch.DESC_DTYPE)["len"] == 20 + 20 + 24).all()
    assert o0[1].tolist() == [batch.V_ACCEPT, batch.V_TCP_HELD, batch.V_TCP_OLD] * 2
    pre = BA.members(RES, fill=77)
    r1, o1 = run(results=pre)
    assert all(a is b for a, b in zip(r1, pre))
    BA._same(r1, r0)
    BA._same(o1, o0)
    r2, o2 = run(results=(None, None))
    assert tuple(r2) == (None, None)
    BA._same(o2, o0)
    r3, o3 = run(**{d: ack_args()[d].view(torch.int64) for d in ("seg_desc", "tmpl_desc", "out_desc", "ack")})
    BA._same(r3, r0)
    BA._same(o3, o0)
    r4, o4 = run(ack=ack_args()["ack"].view(I32))
    BA._same(r4, r0)
