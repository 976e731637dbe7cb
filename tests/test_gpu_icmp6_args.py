"""GPU: the argument checks of picotcp_amd.batch.icmp6_reply_batch, one case per check, as
tests/test_gpu_icmp4_args.py has them for its twin (tests/test_gpu_batch_args.py's faults and its rule: a
rejected call raises ValueError BEFORE the library is reached), on a batch of 2 records (an echo request and
a notice): dtype, length, stride, alignment, device mismatch and flags.  The valid calls pin what the checks
let through."""
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
    return synth.icmp6_burst([synth.icmp6_echo_request(rng, 24, 1, 2), synth.udp6_datagram(rng, 30)], [0, 1], codes=[0, 4])


def icmp_args():
    buf, off, ln, req, ooff, cap, osize = _host()
    return dict(base=to_dev(buf), desc=BA.desc_dev(off, ln), n=N, req=to_dev(req.view(np.uint8)), out=BA.zeros(osize),
                out_desc=BA.desc_dev(ooff, cap))


def misaligned(t, by=8):
    """The same bytes at an address `by` past a 16-byte boundary (a view into a larger tensor)."""
    big = torch.zeros(t.numel() * t.element_size() + 32, dtype=U8, device=t.device)
    v = big[by:by + t.numel() * t.element_size()]
    v.copy_(t.view(U8))
    assert v.data_ptr() % 16 == by
    return v


def misaligned_by_2(t):
    return misaligned(t, 2)


TENSORS = ("base", "desc", "req", "out", "out_desc")
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
    for nm in ("desc", "out_desc", "req"):
        yield arg(nm, BA.one_short)
        yield arg(nm, BA.one_short_int64)
    yield arg("req", BA.strided)
    yield arg("desc", misaligned)
    yield arg("out_desc", misaligned)
    yield arg("req", misaligned_by_2)
    for i in range(len(RES)):
        for fault in (BA.wrong_item_size, BA.one_short, BA.strided, BA.cpu, BA.other_device):
            yield pytest.param("results", i, fault, id=f"results{i}-{fault.__name__}")
    yield pytest.param("results", 1, misaligned, id="results1-misaligned")


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
        batch.icmp6_reply_batch(**kw)


@pytest.mark.parametrize("flags", [_lib.F_WRITE, _lib.F_TX, _lib.F_NXTHDR_DISPATCH, 0x80000000])
def test_flags_are_rejected(flags, monkeypatch):
    monkeypatch.setattr(_lib, "load", BA._no_launch)
    with pytest.raises(ValueError):
        batch.icmp6_reply_batch(**icmp_args(), flags=flags)


def test_missing_verdict_and_negative_count_are_rejected(monkeypatch):
    monkeypatch.setattr(_lib, "load", BA._no_launch)
    with pytest.raises(ValueError):
        batch.icmp6_reply_batch(**icmp_args(), results=(None, BA.zeros(16 * N)))     # the verdicts are required
    kw = icmp_args()
    kw["n"] = -1
    with pytest.raises(ValueError):
        batch.icmp6_reply_batch(**kw)


def test_valid_calls_agree():
    assert batch.icmp6_reply is batch.icmp6_reply_batch

    def run(**over):
        kw = icmp_args()
        kw.update(over)
        res = batch.icmp6_reply_batch(**kw)
        torch.cuda.synchronize()
        return res, [kw["out"]]

    r0, o0 = run()
    assert [(t.dtype, t.numel()) for t in r0] == list(RES)
    assert (r0[0] == batch.V_ACCEPT).all() and r0[1].cpu().numpy().view(batch.DESC_DTYPE)["len"].tolist() == [64, 48 + 78]
    pre = BA.members(RES, fill=77)
    r1, o1 = run(results=pre)
    assert all(a is b for a, b in zip(r1, pre))
    BA._same(r1, r0)
    BA._same(o1, o0)
    r2, o2 = run(results=(pre[0], None))
    assert r2[1] is None
    BA._same(r2[:1], r0[:1])
    BA._same(o2, o0)
    r3, o3 = run(**{d: icmp_args()[d].view(torch.int64) for d in ("desc", "out_desc", "req")})
    BA._same(r3, r0)
    BA._same(o3, o0)
    r4, o4 = run(req=icmp_args()["req"].view(I32))
    BA._same(r4, r0)
    BA._same(o4, o0)
    r5 = batch.icmp6_reply_batch(**{**icmp_args(), "n": 0})            # the empty batch: a no-op
    assert r5[0].numel() == 0
