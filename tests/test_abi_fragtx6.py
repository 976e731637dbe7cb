"""CPU tests of pico_ipv6_fragment_batch_dev's argument checks (include/pico_csum.h): every
refusal comes before any device work, so none of this launches anything."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from picotcp_amd import _lib

vp = ctypes.c_void_p
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pico_csum.h")


def args(**kw):
    """A well-formed call (fake device addresses), fields replaced by keyword."""
    a = dict(d_base=vp(0x1000), base_len=1 << 20, d_dgram=vp(0x2000), n_dgram=4, mtu=1500, d_groups=vp(0x3000), n_frag=16,
             d_out=vp(0x4000), out_len=1 << 20, d_out_desc=vp(0x5000), frag_stride=1504, d_out_frag=vp(0x6000),
             d_out_count=vp(0x7000), d_out_transport=vp(0x8000), d_verdict=vp(0x9000), flags=0, stream=None)
    a.update(kw)
    return tuple(a.values())


def call(**kw):
    return _lib.load().pico_ipv6_fragment_batch_dev(*args(**kw))


def test_symbol_is_exported_and_declared():
    assert "pico_ipv6_fragment_batch_dev" in _lib.EXPORTED
    assert hasattr(_lib.load(), "pico_ipv6_fragment_batch_dev")
    assert _lib.load().pico_csum_abi_version() == 4          # an added entry point: no bump
    text = open(HEADER).read()
    # declared directly behind the IPv4 form, with its argument list
    v4, v6, seg = (text.index(f"int {s}(") for s in ("pico_ipv4_fragment_batch_dev", "pico_ipv6_fragment_batch_dev",
                                                     "pico_tcp_segment_batch_dev"))
    assert v4 < v6 < seg
    decl = lambda at: re.sub(r"\s+", " ", text[at:text.index(";", at)]).split("(", 1)[1]     # noqa: E731
    assert decl(v6) == decl(v4)


@pytest.mark.parametrize("kw", [
    dict(mtu=55), dict(mtu=0), dict(mtu=47),                 # a fragment carries at least 8 payload bytes behind 48
    dict(flags=_lib.F_TX), dict(flags=_lib.F_WRITE | 0x4), dict(flags=_lib.F_NXTHDR_DISPATCH),
    dict(d_dgram=vp(0x2008)), dict(d_groups=vp(0x3002)), dict(d_out_desc=vp(0x5008)), dict(d_out_frag=vp(0x6008)),
    dict(d_out_count=vp(0x7002)), dict(d_out_transport=vp(0x8001)),
    dict(d_base=None), dict(d_out=None), dict(d_dgram=None), dict(d_groups=None), dict(d_out_desc=None),
    dict(frag_stride=1492), dict(frag_stride=1498),          # below 48 + per = 1496; not a multiple of 4
    dict(mtu=1280, frag_stride=1272),                        # per = 1232: at least 1280
    dict(mtu=56, frag_stride=52),
], ids=lambda kw: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in kw.items()))
def test_einval(kw):
    assert call(**kw) == -_lib.EINVAL
    assert _lib.load().pico_csum_last_error().decode() != ""


def test_einval_messages_name_the_bound():
    assert call(mtu=55) == -_lib.EINVAL
    assert "mtu 55" in _lib.load().pico_csum_last_error().decode()
    assert call(mtu=1280, frag_stride=1276) == -_lib.EINVAL
    assert "at least 1280" in _lib.load().pico_csum_last_error().decode()
    assert call(frag_stride=1498) == -_lib.EINVAL
    assert "multiple of 4" in _lib.load().pico_csum_last_error().decode()
    assert call(flags=0x10) == -_lib.EINVAL
    assert "flags 0x10" in _lib.load().pico_csum_last_error().decode()


def test_empty_batch_is_a_no_op():
    assert call(n_dgram=0, d_base=None, d_out=None, d_dgram=None, d_groups=None, d_out_desc=None, mtu=0) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_enodev_without_a_device():
    """No CPU fallback: well-formed arguments without a HIP device give -ENODEV (optional outputs
    NULL, the smallest MTU and stride)."""
    assert call() == -_lib.ENODEV
    assert "HIP device" in _lib.load().pico_csum_last_error().decode()
    assert call(d_out_frag=None, d_out_count=None, d_out_transport=None, d_verdict=None, mtu=56, frag_stride=56,
                flags=_lib.F_WRITE) == -_lib.ENODEV
    assert call(mtu=1280, frag_stride=1280) == -_lib.ENODEV
