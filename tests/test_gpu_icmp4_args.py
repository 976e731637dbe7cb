"""GPU: the argument checks of picotcp_amd.batch.icmp4_reply_batch, one case per check, as
tests/test_gpu_batch_args.py has them for the other wrappers (its faults and its rule: a rejected call
raises ValueError BEFORE the library is reached), on a batch of 2 records (an echo request and a
notice).  The valid calls pin what the checks let through."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from picotcp_amd import _lib, batch, synth
from tests import test_gpu_batch_args as BA
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu

N = BA.N
U8, I32 = torch.uint8, torch.int32


@functools.lru_cache(maxsize=None)
def _host():
    rng = np.random.default_rng(8)
    return synth.icmp4_burst([synth.icmp4_echo_request(rng, 24, 1, 2), synth.icmp4_echo_request(rng, 30, 3, 4)], [0, 11])


def icmp_args():
    buf, off, ln, req, ooff, cap, osize = _host()
    return dict(base=to_dev(buf), desc=BA.desc_dev(off, ln), n=N, req=to_dev(req.view(np.uint8)), out=BA.zeros(osize),
                out_desc=BA.desc_dev(ooff, cap), state=batch.icmp4_state(BA.DEV))


TENSORS = ("base", "desc", "req", "out", "out_desc", "state")
RES = ((U8, N), (U8, 16 * N))


def _cases():
    def arg(name, fault):
        return pytest.param(name, None, fault, id=f"{name}-{fault.__name__}")

    for nm in TENSORS:
        yield arg(nm, BA.cpu)
        yield arg(nm, BA.other_device)
    for nm in ("base", "out"):
        yield arg(nm, BA.not_u8)
        yield arg(nm, BA.strided)
    for nm in ("desc", "out_desc", "req", "state"):
        yield arg(nm, BA.one_short)
        yield arg(nm, BA.one_short_int64)
    for nm in ("req", "state"):
        yield arg(nm, BA.strided)
    for i in range(len(RES)):
        for fault in (BA.wrong_item_size, BA.one_short, BA.strided, BA.cpu, BA.other_device):
            yield pytest.param("results", i, fault, id=f"results{i}-{fault.__name__}")


@pytest.mark.parametrize("name,member,fault", list(_cases()))
def test_rejected_before_the_launch(name, member, fault, monkeypatch):
    if fault is BA.other_device and torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    kw = icmp_args()
    if member is None:
        kw[name] = fault(kw[name])
    else:
        res = list(BA.members(RES))
        res[member] = fault(res[member])
        kw["results"] = tuple(res)
    monkeypatch.setattr(_lib, "load", BA._no_launch)
    with pytest.raises(ValueError):
        batch.icmp4_reply_batch(**kw)


def test_missing_verdict_and_negative_count_are_rejected(monkeypatch):
    monkeypatch.setattr(_lib, "load", BA._no_launch)
    with pytest.raises(ValueError):
        batch.icmp4_reply_batch(**icmp_args(), results=(None, BA.zeros(16 * N)))     # the verdicts are required
    kw = icmp_args()
    kw["n"] = -1
    with pytest.raises(ValueError):
        batch.icmp4_reply_batch(**kw)


def test_valid_calls_agree():
    def run(**over):
        kw = icmp_args()
        kw.update(over)
        res = batch.icmp4_reply_batch(**kw)
        torch.cuda.synchronize()
        return res, [kw["out"]] + ([kw["state"]] if kw["state"] is not None else [])

    r0, o0 = run()
    assert [(t.dtype, t.numel()) for t in r0] == list(RES)
    assert (r0[0] == batch.V_ACCEPT).all() and r0[1].cpu().numpy().view(batch.DESC_DTYPE)["len"].tolist() == [44, 56]
    assert o0[1].cpu().numpy().view(batch.ICMP4_STATE_DTYPE)[0].tolist() == (1, 0x0100, 0x0200)
    pre = BA.members(RES, fill=77)
    r1, o1 = run(results=pre)
    assert all(a is b for a, b in zip(r1, pre))
    BA._same(r1, r0)
    BA._same(o1, o0)
    r2, o2 = run(results=(pre[0], None))
    assert r2[1] is None
    BA._same(r2[:1], r0[:1])
    BA._same(o2, o0)
    r3, o3 = run(**{d: icmp_args()[d].view(torch.int64) for d in ("desc", "out_desc", "req", "state")})
    BA._same(r3, r0)
    BA._same(o3[:1], o0[:1])
    r4, o4 = run(req=icmp_args()["req"].view(I32), state=None)
    BA._same(r4, r0)
    BA._same(o4, o0[:1])
    r5 = batch.icmp4_reply_batch(**{**icmp_args(), "n": 0})            # the empty batch: a no-op
    assert r5[0].numel() == 0
