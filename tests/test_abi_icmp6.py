"""CPU tests of pico_icmp6_reply_batch_dev's ABI and argument checks (include/pico_csum.h): every refusal
comes before any device work, so none of this launches anything."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from picotcp_amd import _lib, batch
from tests import icmp6_ref as I

vp = ctypes.c_void_p
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "pico_csum.h")


def args(**kw):
    """A well-formed call (fake device addresses), fields replaced by keyword."""
    a = dict(d_base=vp(0x1000), base_len=1 << 20, d_desc=vp(0x2000), n=4, d_req=vp(0x3000), d_out=vp(0x4000),
             out_len=1 << 20, d_out_desc=vp(0x5000), d_out_ans=vp(0x6000), d_verdict=vp(0x7000), flags=0, stream=None)
    a.update(kw)
    return tuple(a.values())


def call(**kw):
    return _lib.load().pico_icmp6_reply_batch_dev(*args(**kw))


def test_symbol_is_exported_and_declared():
    assert "pico_icmp6_reply_batch_dev" in _lib.EXPORTED
    assert hasattr(_lib.load(), "pico_icmp6_reply_batch_dev")
    src = open(HEADER).read()
    assert re.search(r"\bint pico_icmp6_reply_batch_dev\(", src)
    assert "4 (added, no bump): pico_icmp6_reply_batch_dev" in src
    m = re.search(r"int pico_icmp6_reply_batch_dev\((.*?)\);", src, re.S)
    assert "state" not in m.group(1)                             # the reference keeps none for ICMPv6


def test_abi_version_is_still_4():
    assert _lib.load().pico_csum_abi_version() == _lib.ABI_VERSION == 4          # an added entry point: no bump
    assert "#define PICO_CSUM_ABI_VERSION 4" in open(HEADER).read()


def test_struct_size_and_offsets():
    """struct pico_csum_icmp6_req: 24 bytes, src 0, arg 16, type 20, code 21, hop 22, rsvd 23 -- in the header,
    the binding and the restatement."""
    src = open(HEADER).read()
    m = re.search(r"struct pico_csum_icmp6_req \{(.*?)\};", src, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    size = {"uint32_t": 4, "uint16_t": 2, "uint8_t": 1}
    fields, off = [], 0
    for t, group in re.findall(r"(uint\d+_t)\s+([a-z0-9_,\[\] ]+);", body):
        for f in group.split(","):
            f = f.strip()
            k = re.fullmatch(r"(\w+)\[(\d+)\]", f)
            nbytes = size[t] * (int(k.group(2)) if k else 1)
            assert off % size[t] == 0                            # naturally aligned: no padding
            fields.append((k.group(1) if k else f, off, nbytes))
            off += nbytes
    assert fields == [("src", 0, 16), ("arg", 16, 4), ("type", 20, 1), ("code", 21, 1), ("hop", 22, 1), ("rsvd", 23, 1)]
    assert off == 24
    for dt in (batch.ICMP6_REQ_DTYPE, I.REQ_DTYPE):
        assert dt.itemsize == 24 and dt.names == tuple(f for f, _, _ in fields)
        assert [(dt.fields[f][1], dt.fields[f][0].itemsize) for f in dt.names] == [(o, s) for _, o, s in fields]


@pytest.mark.parametrize("kw", [
    dict(flags=_lib.F_WRITE), dict(flags=_lib.F_TX), dict(flags=0x4), dict(flags=_lib.F_NXTHDR_DISPATCH),
    dict(flags=0x80000000),                                  # reserved: anything but 0
    dict(d_desc=vp(0x2008)), dict(d_out_desc=vp(0x5008)), dict(d_out_ans=vp(0x6008)),
    dict(d_req=vp(0x3002)),
    dict(d_base=None), dict(d_desc=None), dict(d_req=None), dict(d_out=None), dict(d_out_desc=None), dict(d_verdict=None),
], ids=lambda kw: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in kw.items()))
def test_einval(kw):
    assert call(**kw) == -_lib.EINVAL
    assert _lib.load().pico_csum_last_error().decode() != ""


def test_empty_batch_is_a_no_op():
    assert call(n=0, d_base=None, d_desc=None, d_req=None, d_out=None, d_out_desc=None, d_out_ans=None, d_verdict=None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_enodev_without_a_device():
    """No CPU fallback: well-formed arguments without a HIP device give -ENODEV (also with the optional
    pointer NULL)."""
    assert call() == -_lib.ENODEV
    assert "HIP device" in _lib.load().pico_csum_last_error().decode()
    assert call(d_out_ans=None) == -_lib.ENODEV
