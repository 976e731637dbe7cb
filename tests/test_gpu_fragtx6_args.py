"""GPU: the argument checks of batch.ipv6_fragment_batch, one case per check, on a batch of 2 datagrams
with 3 fragments each -- the grid of tests/test_gpu_batch_args.py (its faults and its no-launch guard,
imported) for the wrapper that file does not list.  A rejected call must raise ValueError BEFORE the
library is reached; the valid calls pin what the checks let through."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from picotcp_amd import _lib, batch, synth
from tests import test_gpu_batch_args as A
from tests.gpu_util import DEV, pairs_dev, to_dev

pytestmark = pytest.mark.gpu

N, M = A.N, A.M
TENSORS = ("base", "dgram_desc", "groups", "out", "out_desc")
DESCS = {"dgram_desc": N, "out_desc": N}
RES_SPEC = ((A.U8, N), (A.I32, N), (A.I16, N))


@functools.lru_cache(maxsize=None)
def _host():
    r = synth.ipv6_oversized([40, 48], mtu=64, stride=64, seed=6)       # per 16: 3 fragments each
    assert r[7] == M
    return r


def make():
    buf, off, dlen, ids, groups, ooff, cap, n_frag, out_size = _host()
    return dict(base=to_dev(buf), dgram_desc=A.desc_dev(off, dlen, ids), mtu=64, groups=pairs_dev(groups), n_frag=M,
                out=A.zeros(out_size), out_desc=A.desc_dev(ooff, cap), frag_stride=64, flags=batch.F_WRITE,
                out_frag=A.zeros(16 * M))


def _cases():
    def arg(name, fault):
        return pytest.param(name, None, fault, id=f"{name}-{fault.__name__}")

    for nm in TENSORS:
        yield arg(nm, A.cpu)
        yield arg(nm, A.other_device)
    for nm in ("base", "out"):
        yield arg(nm, A.not_u8)
        yield arg(nm, A.strided)
    yield arg("groups", A.eight_byte)
    yield arg("groups", A.strided)
    for nm in DESCS:
        yield arg(nm, A.one_short)
        yield arg(nm, A.one_short_int64)
    for fault in (A.one_short, A.one_short_int64, A.strided, A.cpu, A.other_device):
        yield arg("out_frag", fault)
    for i in range(len(RES_SPEC)):
        for fault in (A.wrong_item_size, A.one_short, A.strided, A.cpu, A.other_device):
            yield pytest.param("results", i, fault, id=f"results{i}-{fault.__name__}")


@pytest.mark.parametrize("name,member,fault", list(_cases()))
def test_rejected_before_the_launch(name, member, fault, monkeypatch):
    if fault is A.other_device and torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    kw = make()
    if member is None:
        kw[name] = fault(kw[name])
    else:
        res = list(A.members(RES_SPEC))
        res[member] = fault(res[member])
        kw["results"] = tuple(res)
    monkeypatch.setattr(_lib, "load", A._no_launch)
    with pytest.raises(ValueError):
        batch.ipv6_fragment_batch(**kw)


@pytest.mark.parametrize("over", [dict(mtu=55), dict(frag_stride=62), dict(frag_stride=60), dict(flags=batch.F_TX)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_library_refusals_surface_as_errors(over):
    """What only the library checks (the MTU, the stride, the flags) comes back as PicoCsumError, -EINVAL."""
    kw = make()
    kw.update(over)
    with pytest.raises(_lib.PicoCsumError) as e:
        batch.ipv6_fragment_batch(**kw)
    assert e.value.rc == -_lib.EINVAL


def test_valid_calls_agree():
    def run(**over):
        kw = make()
        kw.update(over)
        res = batch.ipv6_fragment_batch(**kw)
        torch.cuda.synchronize()
        return res, [kw[k] for k in ("out", "out_frag") if kw.get(k) is not None]

    r0, o0 = run()
    assert [(t.dtype, t.numel()) for t in r0] == list(RES_SPEC)
    assert (r0[0] == batch.V_ACCEPT).all() and r0[1].tolist() == [3, 3]
    pre = A.members(RES_SPEC, fill=77)
    r1, o1 = run(results=pre)
    assert all(a is b for a, b in zip(r1, pre))
    A._same(r1, r0)
    A._same(o1, o0)
    r2, o2 = run(results=(None, None, None), out_frag=None)
    assert tuple(r2) == (None, None, None)
    A._same(o2, o0[:1])
    r3, o3 = run(**{d: make()[d].view(torch.int64) for d in DESCS})
    A._same(r3, r0)
    A._same(o3, o0)
    assert np.array_equal(o0[1].cpu().numpy().view(batch.DESC_DTYPE)["len"], [64, 64, 56, 64, 64, 64])
