"""Host-side (Python) mirror of the batched checksum API over torch device tensors.

Each function is a thin call into libpicocsum.so (include/pico_csum.h); the
work happens in the HIP kernels.  Frame buffers are uint8 tensors on a HIP
device; descriptor arrays are uint8 tensors of n*16 bytes (struct
pico_csum_desc); results are int16 tensors holding the uint16 checksum bits
(view them as uint16 with `.cpu().numpy().view(np.uint16)`).

Reference interfaces mirrored (per frame in the reference, per batch here):
  checksum_uniform / checksum_batch  <- pico_checksum, pico_dualbuffer_checksum
                                        (stack/pico_frame.c:312-328)
  ipv4_checksum_batch                <- pico_ipv4_checksum / pico_ipv4_crc_check
                                        (modules/pico_ipv4.c:231-257), pico_ipv4_process_in
                                        (:381-456: source, evil bit, IHL, fragments),
                                        pico_tcp_checksum_ipv4 (pico_tcp.c:422),
                                        pico_udp_checksum_ipv4 (pico_udp.c:36),
                                        pico_icmp4_checksum (pico_icmp4.c:30),
                                        pico_transport_crc_check (pico_socket.c:1916)
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import (F_NXTHDR_DISPATCH, F_TX, F_WRITE, FLOW_F_ETH, FLOW_FRAG4, FLOW_FRAG6, FLOW_TCP, V_ACCEPT, V_ARP, V_DROP_L2, V_DUPLICATE,  # noqa: F401
                   V_EXPIRED, V_FRAG, V_IPV6, V_L4_BAD, V_LOCAL_SRC, V_MALFORMED, V_NET_BAD, V_TCP_CTRL, V_TCP_HELD,
                   V_TCP_OLD, V_UNTOUCHED)

DESC_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("seed", "<u4")])
# struct pico_csum_nat (include/pico_csum.h): the NAT batch's per-datagram record
NAT_DTYPE = np.dtype([("addr", "<u4"), ("port", "<u2"), ("dir", "u1"), ("reserved", "u1")])
NAT_NONE, NAT_OUTBOUND, NAT_INBOUND = 0, 1, 2
assert DESC_DTYPE.itemsize == 16


def make_desc(offsets, lengths, seeds=None) -> np.ndarray:
    """Host descriptor array (struct pico_csum_desc[n])."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    d = np.zeros(offsets.shape[0], dtype=DESC_DTYPE)
    d["off"] = offsets
    d["len"] = np.asarray(lengths, dtype=np.uint32)
    if seeds is not None:
        d["seed"] = np.asarray(seeds, dtype=np.uint32)
    return d


def desc_to_device(desc: np.ndarray, device) -> torch.Tensor:
    """Copy a descriptor array to the device (fresh allocation: 16-B aligned)."""
    raw = np.ascontiguousarray(desc).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy()).to(device)


def _stream_handle(stream) -> ctypes.c_void_p:
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def _ptr(t: torch.Tensor | None) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a HIP device tensor (the batched path is GPU-only)")


def _check_out(out: torch.Tensor, n: int, name: str, device, itemsize: int = 2) -> None:
    """A caller-supplied result tensor: on the batch's device (a HIP device: `base` is on it),
    contiguous, the right element size and at least n elements (the kernels write n results through
    its pointer)."""
    if out.device != device:
        raise ValueError(f"{name} is on {out.device}, the batch on {device}")
    if not out.is_contiguous() or out.element_size() != itemsize:
        raise ValueError(f"{name} must be a contiguous tensor of {itemsize}-byte elements")
    if out.numel() < n:
        raise ValueError(f"{name} has {out.numel()} elements, the batch {n}")


def _require_u8(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous uint8 tensor")


def _on_batch_device(base: torch.Tensor, **tensors):
    """`base` is a device tensor and every named tensor is on its device, which is returned."""
    _require_device(base, "base")
    dev = base.device
    for name, t in tensors.items():
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the batch on {dev}")
    return dev


def _pairs(t: torch.Tensor, name: str, n: int | None = None) -> int:
    """A contiguous tensor of 4-byte elements holding one pair per group; returns the pairs it holds.
    n=None is the tensor the batch takes its group count FROM (`groups`: n = numel // 2, so no count
    could be wrong); n given is a tensor that must hold a pair for each of those n groups (`conn`)."""
    if t.element_size() != 4 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 32-bit tensor of one pair per group")
    if n is not None and t.numel() < 2 * n:
        raise ValueError(f"{name} holds {t.numel() // 2} pairs, the batch has {n} groups")
    return t.numel() // 2


def _desc_bytes(t: torch.Tensor, count: int, name: str, by_element: bool = False) -> None:
    """A descriptor tensor of at least 16 * count bytes.  by_element: the rule of the wrappers older than
    the scatter/gather batches, 16 * count ELEMENTS -- the same thing for a uint8 tensor, 8 times the
    bytes for an int64 one.  It is kept as those wrappers have it, not folded into the byte rule."""
    if (t.numel() if by_element else t.numel() * t.element_size()) < 16 * count:
        raise ValueError(f"{name} is shorter than {count} 16-byte descriptors")


def _opt_desc_out(t: torch.Tensor | None, count: int, name: str, device) -> None:
    """The optional descriptor output of a scatter batch (out_frag / out_seg), when given."""
    if t is None:
        return
    if t.device != device or not t.is_contiguous() or t.numel() * t.element_size() < 16 * count:
        raise ValueError(f"{name} must be a contiguous tensor of {count} 16-byte descriptors on the batch's device")


def _results(results, spec, counts, device) -> tuple:
    """A wrapper's result tensors, in return order: spec = (name, dtype, itemsize, optional) per member
    (a constant beside its wrapper), counts = each member's elements.  None allocates them all; a
    caller's own are checked (_check_out), an optional member may be None (the library skips that
    output)."""
    if results is None:
        return tuple(torch.empty(count, dtype=dtype, device=device) for (_, dtype, _, _), count in zip(spec, counts))
    for t, (name, _, itemsize, optional), count in zip(results, spec, counts):
        if t is not None or not optional:
            _check_out(t, count, name, device, itemsize)
    return results if type(results) is tuple else tuple(results)


# the fused checksum batches' (out_net, out_transport, verdict); the IPv6 batch returns the last two
_CHECKSUM_OUTS = (("out_net", torch.int16, 2, False), ("out_transport", torch.int16, 2, False), ("verdict", torch.uint8, 1, False))
_CHECKSUM6_OUTS = _CHECKSUM_OUTS[1:]


def checksum_uniform(base: torch.Tensor, stride: int, length: int, n: int, seed: int = 0,
                     out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """out[i] = pico_checksum(base + i*stride, length) (+ seed as pico_dualbuffer_checksum's
    first buffer); device-resident, asynchronous on `stream`."""
    _require_device(base, "base")
    if n and (n - 1) * stride + length > base.numel():
        raise ValueError("frames exceed the base tensor")
    if out is None:
        out = torch.empty(n, dtype=torch.int16, device=base.device)
    _check_out(out, n, "out", base.device)
    lib = _lib.load()
    _lib.check("pico_checksum_batch_uniform_dev",
               lib.pico_checksum_batch_uniform_dev(_ptr(base), base.numel(), stride, length, n, seed & 0xFFFFFFFF,
                                                   _ptr(out), _stream_handle(stream)))
    return out


def checksum_batch(base: torch.Tensor, desc: torch.Tensor, n: int, crc_off: int = -1, flags: int = 0,
                   out: torch.Tensor | None = None, bad: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """out[i] = finalize(adder(desc[i].seed, base + desc[i].off, desc[i].len)); crc field
    at crc_off read as zero (and written with F_WRITE).  Regions outside `base` are not
    read (out 0); `bad` (int32[1] on the device) counts them when given."""
    _require_device(base, "base")
    _require_device(desc, "desc")
    _desc_bytes(desc, n, "desc", by_element=True)
    if out is None:
        out = torch.empty(n, dtype=torch.int16, device=base.device)
    _check_out(out, n, "out", base.device)
    if bad is not None:
        _check_out(bad, 1, "bad", base.device, itemsize=4)
    lib = _lib.load()
    _lib.check("pico_checksum_batch_dev",
               lib.pico_checksum_batch_dev(_ptr(base), base.numel(), _ptr(desc), n, crc_off, flags, _ptr(out),
                                           _ptr(bad), _stream_handle(stream)))
    return out


def ipv4_checksum_batch(base: torch.Tensor, desc: torch.Tensor, n: int, flags: int = 0, stream=None, out=None):
    """Fused IPv4 header + transport checksums (RX verify, or TX compute with F_TX).
    Returns (out_net int16[n], out_transport int16[n], verdict uint8[n]); `out` may pass
    that triple preallocated."""
    _require_device(base, "base")
    _require_device(desc, "desc")
    _desc_bytes(desc, n, "desc", by_element=True)
    out_net, out_l4, verdict = _results(out, _CHECKSUM_OUTS, (n, n, n), base.device)
    lib = _lib.load()
    _lib.check("pico_ipv4_checksum_batch_dev",
               lib.pico_ipv4_checksum_batch_dev(_ptr(base), base.numel(), _ptr(desc), n, flags, _ptr(out_net),
                                                _ptr(out_l4), _ptr(verdict), _stream_handle(stream)))
    return out_net, out_l4, verdict


def ipv6_checksum_batch(base: torch.Tensor, desc: torch.Tensor, n: int, flags: int = 0, stream=None, out=None):
    """Fused IPv6 transport checksums (TCP / UDP / ICMPv6; RX verify, or TX compute with
    F_TX).  desc.seed = net_len | proto << 16 (0: no extension headers).
    Returns (out_transport int16[n], verdict uint8[n]); `out` may pass that pair
    preallocated."""
    _require_device(base, "base")
    _require_device(desc, "desc")
    _desc_bytes(desc, n, "desc", by_element=True)
    out_l4, verdict = _results(out, _CHECKSUM6_OUTS, (n, n), base.device)
    lib = _lib.load()
    _lib.check("pico_ipv6_checksum_batch_dev",
               lib.pico_ipv6_checksum_batch_dev(_ptr(base), base.numel(), _ptr(desc), n, flags, _ptr(out_l4),
                                                _ptr(verdict), _stream_handle(stream)))
    return out_l4, verdict


_MACS: dict = {}


def _mac_buf(mac: bytes):
    """A ctypes copy of a 6-byte MAC, built once per address (launch overhead stays below the kernel's)."""
    b = _MACS.get(mac)
    if b is None:
        b = _MACS[mac] = ctypes.create_string_buffer(mac, 6)
    return b


def eth_checksum_batch(base: torch.Tensor, desc: torch.Tensor, n: int, flags: int = 0, mac: bytes | None = None,
                       stream=None, out=None):
    """Ethernet front end + fused IPv4 / IPv6 checksums in one launch (pico_ethernet.c:180-235):
    desc.off -> Ethernet header, desc.len = frame bytes, desc.seed = IPv6 net_len | proto << 16.
    mac = the device address (6 bytes) for the RX destination filter, None = no filter.
    Returns (out_net int16[n], out_transport int16[n], verdict uint8[n])."""
    _require_device(base, "base")
    _require_device(desc, "desc")
    _desc_bytes(desc, n, "desc", by_element=True)
    if mac is not None and len(mac) != 6:
        raise ValueError("mac must be 6 bytes")
    out_net, out_l4, verdict = _results(out, _CHECKSUM_OUTS, (n, n, n), base.device)
    lib = _lib.load()
    m = None if mac is None else _mac_buf(bytes(mac))
    _lib.check("pico_eth_checksum_batch_dev",
               lib.pico_eth_checksum_batch_dev(_ptr(base), base.numel(), _ptr(desc), n, flags, m, _ptr(out_net),
                                               _ptr(out_l4), _ptr(verdict), _stream_handle(stream)))
    return out_net, out_l4, verdict


FWD_STATE_BYTES = 16          # struct pico_csum_fwd_state


def fwd_state(device) -> torch.Tensor:
    """A forwarding state (struct pico_csum_fwd_state) at the reference's initial value (zeros)."""
    return torch.zeros(FWD_STATE_BYTES, dtype=torch.uint8, device=device)


def ipv4_forward_batch(base: torch.Tensor, desc: torch.Tensor, n: int, *, state: torch.Tensor | None, local=(),
                       verdict: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """pico_ipv4_pre_forward_checks (pico_ipv4.c:1535-1574) in batch order, in place on n datagrams:
    ttl - 1, then unless the TTL expired the reference's crc++, the local-source check against
    `local` (the host's link addresses as stored: uint32 little-endian views, <= 32) and the
    duplicate check against the last forwarded tuple, carried in `state` (fwd_state()).  `state`
    is required: a sequence split over several calls must pass the same state tensor to each, as
    the reference's statics carry the last tuple; `state=None` is the explicit one-shot mode (the
    reference's zero initial state, nothing kept).  Descriptors of one batch must not overlap
    (two descriptors on one header would race on its TTL / crc).  Returns the verdicts (V_ACCEPT
    = forwarded, V_EXPIRED, V_LOCAL_SRC, V_DUPLICATE, V_MALFORMED)."""
    _require_device(base, "base")
    _require_u8(base, "base")
    _require_device(desc, "desc")
    _desc_bytes(desc, n, "desc", by_element=True)
    if verdict is None:
        verdict = torch.empty(n, dtype=torch.uint8, device=base.device)
    _check_out(verdict, n, "verdict", base.device, 1)
    if state is not None:
        _require_device(state, "state")
        if state.numel() * state.element_size() < FWD_STATE_BYTES or not state.is_contiguous():
            raise ValueError("state must be a contiguous 16-byte tensor (fwd_state())")
    loc = np.ascontiguousarray(np.asarray(local, dtype=np.uint32))
    lib = _lib.load()
    _lib.check("pico_ipv4_forward_batch_dev",
               lib.pico_ipv4_forward_batch_dev(_ptr(base), base.numel(), _ptr(desc), n,
                                               loc.ctypes.data if loc.size else None, loc.size,
                                               _ptr(state) if state is not None else None, _ptr(verdict),
                                               _stream_handle(stream)))
    return verdict


def ipv4_nat_batch(base: torch.Tensor, desc: torch.Tensor, n: int, nat: torch.Tensor, stream=None, out=None):
    """NAT rewrite (pico_ipv4_nat_outbound / _inbound's frame work, pico_nat.c:424-545) in place on
    n IPv4 datagrams: nat = 8-byte records {addr u32, port u16, dir u8, 0} as uint8 / int64 tensor
    (NAT_DTYPE layout).  Returns (out_net int16[n], out_transport int16[n], verdict uint8[n]):
    V_ACCEPT translated, V_UNTOUCHED, V_FRAG, V_MALFORMED."""
    _require_device(base, "base")
    _require_u8(base, "base")
    _require_device(desc, "desc")
    _require_device(nat, "nat")
    _desc_bytes(desc, n, "desc", by_element=True)
    if nat.numel() * nat.element_size() < 8 * n or not nat.is_contiguous():
        raise ValueError("nat must be a contiguous tensor of n 8-byte records")
    out_net, out_l4, verdict = _results(out, _CHECKSUM_OUTS, (n, n, n), base.device)
    lib = _lib.load()
    _lib.check("pico_ipv4_nat_batch_dev",
               lib.pico_ipv4_nat_batch_dev(_ptr(base), base.numel(), _ptr(desc), n, _ptr(nat), _ptr(out_net),
                                           _ptr(out_l4), _ptr(verdict), _stream_handle(stream)))
    return out_net, out_l4, verdict


def ipv4_reassemble_batch(base: torch.Tensor, frag_desc: torch.Tensor, n_frag: int, groups: torch.Tensor,
                          out: torch.Tensor, out_desc: torch.Tensor, stream=None, results=None):
    """IPv4 reassembly gather + transport check (pico_fragments.c:216-358): groups = uint32
    (first, count) pairs per datagram (int32 tensor of 2*n), out = uint8 device buffer the
    datagrams are written into at out_desc[g].off.  Returns (out_len int32[n], out_transport
    int16[n], verdict uint8[n])."""
    return _reassemble(False, base, frag_desc, n_frag, groups, out, out_desc, 0, stream, results)


def ipv6_reassemble_batch(base: torch.Tensor, frag_desc: torch.Tensor, n_frag: int, groups: torch.Tensor,
                          out: torch.Tensor, out_desc: torch.Tensor, flags: int = 0, stream=None, results=None):
    """IPv6 reassembly gather + transport check (pico_fragments.c:432-498, 304-358): as
    ipv4_reassemble_batch, descriptors at each fragment's IPv6 header; flags F_NXTHDR_DISPATCH."""
    return _reassemble(True, base, frag_desc, n_frag, groups, out, out_desc, flags, stream, results)


_REASSEMBLE_OUTS = (("out_len", torch.int32, 4, False), ("out_transport", torch.int16, 2, False), ("verdict", torch.uint8, 1, False))


def _reassemble(v6, base, frag_desc, n_frag, groups, out, out_desc, flags, stream, results):
    dev = _on_batch_device(base, frag_desc=frag_desc, groups=groups, out=out, out_desc=out_desc)
    _require_u8(base, "base")
    _require_u8(out, "out")
    n = _pairs(groups, "groups")
    _desc_bytes(frag_desc, n_frag, "frag_desc")
    _desc_bytes(out_desc, n, "out_desc")
    ol, l4, v = _results(results, _REASSEMBLE_OUTS, (n, n, n), dev)
    lib = _lib.load()
    if v6:
        _lib.check("pico_ipv6_reassemble_batch_dev",
                   lib.pico_ipv6_reassemble_batch_dev(_ptr(base), base.numel(), _ptr(frag_desc), n_frag, _ptr(groups),
                                                      n, _ptr(out), out.numel(), _ptr(out_desc), _ptr(ol), _ptr(l4),
                                                      _ptr(v), flags, _stream_handle(stream)))
    else:
        _lib.check("pico_ipv4_reassemble_batch_dev",
                   lib.pico_ipv4_reassemble_batch_dev(_ptr(base), base.numel(), _ptr(frag_desc), n_frag, _ptr(groups),
                                                      n, _ptr(out), out.numel(), _ptr(out_desc), _ptr(ol), _ptr(l4),
                                                      _ptr(v), _stream_handle(stream)))
    return ol, l4, v


_FRAGMENT_OUTS = (("verdict", torch.uint8, 1, True), ("count", torch.int32, 4, True), ("out_transport", torch.int16, 2, True))
_SEGMENT_OUTS = _FRAGMENT_OUTS[:2]


def ipv4_fragment_batch(base: torch.Tensor, dgram_desc: torch.Tensor, mtu: int, groups: torch.Tensor, n_frag: int,
                        out: torch.Tensor, out_desc: torch.Tensor, frag_stride: int, flags: int = 0,
                        out_frag: torch.Tensor | None = None, stream=None, results=None):
    """IPv4 TX fragmentation scatter + header checksums + the whole datagram's transport checksum
    (pico_socket_xmit_fragments, pico_socket.c:1131-1251; pico_ipv4_frame_push, pico_ipv4.c:1039-1079):
    the inverse of ipv4_reassemble_batch.  dgram_desc = one unfragmented datagram per descriptor
    (20-byte header + transport), groups = uint32 (first slot, slots reserved) pairs per datagram
    (int32 tensor of 2*n), out = uint8 device buffer; fragment k of datagram g is written at
    out_desc[g].off + k*frag_stride, per = (mtu - 20) & ~7 payload bytes each.  out_frag (uint8
    tensor of 16*n_frag bytes, or None) receives the fragments' descriptors.  flags: F_WRITE stores
    the transport checksum into its crc field.  Returns (verdict uint8[n], count int32[n],
    out_transport int16[n]); `results` may pass that triple preallocated, any of them None to skip it."""
    dev = _on_batch_device(base, dgram_desc=dgram_desc, groups=groups, out=out, out_desc=out_desc)
    _require_u8(base, "base")
    _require_u8(out, "out")
    n = _pairs(groups, "groups")
    _desc_bytes(dgram_desc, n, "dgram_desc")
    _desc_bytes(out_desc, n, "out_desc")
    _opt_desc_out(out_frag, n_frag, "out_frag", dev)
    v, cnt, l4 = _results(results, _FRAGMENT_OUTS, (n, n, n), dev)
    lib = _lib.load()
    _lib.check("pico_ipv4_fragment_batch_dev",
               lib.pico_ipv4_fragment_batch_dev(_ptr(base), base.numel(), _ptr(dgram_desc), n, mtu, _ptr(groups), n_frag,
                                                _ptr(out), out.numel(), _ptr(out_desc), frag_stride, _ptr(out_frag),
                                                _ptr(cnt), _ptr(l4), _ptr(v), flags, _stream_handle(stream)))
    return v, cnt, l4


def ipv6_fragment_batch(base: torch.Tensor, dgram_desc: torch.Tensor, mtu: int, groups: torch.Tensor, n_frag: int,
                        out: torch.Tensor, out_desc: torch.Tensor, frag_stride: int, flags: int = 0,
                        out_frag: torch.Tensor | None = None, stream=None, results=None):
    """IPv6 TX fragmentation scatter + the whole datagram's transport checksum (RFC 8200 4.5; the
    reference cannot fragment IPv6, pico_socket.c:1179-1185, but reassembles what this writes,
    pico_fragments.c:432-498): the inverse of ipv6_reassemble_batch.  As ipv4_fragment_batch, with
    dgram_desc = one unfragmented datagram per descriptor (40-byte fixed header + transport, no
    extension headers; seed = the 32-bit fragment identification), per = (mtu - 48) & ~7 payload
    bytes behind 48 header bytes a fragment, frag_stride >= 48 + per; a datagram of len <= mtu goes
    out whole, without a fragment header.  flags: F_WRITE stores the transport checksum into its crc
    field.  Returns (verdict uint8[n], count int32[n], out_transport int16[n]); `results` may pass
    that triple preallocated, any of them None to skip it."""
    dev = _on_batch_device(base, dgram_desc=dgram_desc, groups=groups, out=out, out_desc=out_desc)
    _require_u8(base, "base")
    _require_u8(out, "out")
    n = _pairs(groups, "groups")
    _desc_bytes(dgram_desc, n, "dgram_desc")
    _desc_bytes(out_desc, n, "out_desc")
    _opt_desc_out(out_frag, n_frag, "out_frag", dev)
    v, cnt, l4 = _results(results, _FRAGMENT_OUTS, (n, n, n), dev)
    lib = _lib.load()
    _lib.check("pico_ipv6_fragment_batch_dev",
               lib.pico_ipv6_fragment_batch_dev(_ptr(base), base.numel(), _ptr(dgram_desc), n, mtu, _ptr(groups), n_frag,
                                                _ptr(out), out.numel(), _ptr(out_desc), frag_stride, _ptr(out_frag),
                                                _ptr(cnt), _ptr(l4), _ptr(v), flags, _stream_handle(stream)))
    return v, cnt, l4


def tcp_segment_batch(base: torch.Tensor, stream_desc: torch.Tensor, groups: torch.Tensor, n_seg: int,
                      out: torch.Tensor, out_desc: torch.Tensor, seg_stride: int, flags: int = 0,
                      out_seg: torch.Tensor | None = None, stream=None, results=None):
    """TCP send segmentation + every frame's IPv4 header checksum and TCP checksum in one pass
    (pico_socket_xmit, pico_socket.c:1322-1358; pico_tcp_push / tcp_send, pico_tcp.c:3127-3157, :968-985;
    pico_ipv4_frame_push, pico_ipv4.c:1039-1079).  stream_desc = one send unit per descriptor: off ->
    IPv4 (IHL 5) or IPv6 header + TCP header + payload, len = all of it, seed = payload bytes a
    segment; groups = uint32 (first slot, slots reserved) pairs per stream (int32 tensor of 2*n), out =
    uint8 device buffer; segment k of stream g is written at out_desc[g].off + k*seg_stride with its
    own len / id + k / seq + k*per and checksums.  out_seg (uint8 tensor of 16*n_seg bytes, or None)
    receives the segments' descriptors -- with `out`, the input of ipv4_checksum_batch /
    ipv6_checksum_batch.  flags: reserved, 0.  Returns (verdict uint8[n], count int32[n]); `results`
    may pass that pair preallocated, either of them None to skip it."""
    dev = _on_batch_device(base, stream_desc=stream_desc, groups=groups, out=out, out_desc=out_desc)
    _require_u8(base, "base")
    _require_u8(out, "out")
    n = _pairs(groups, "groups")
    _desc_bytes(stream_desc, n, "stream_desc")
    _desc_bytes(out_desc, n, "out_desc")
    _opt_desc_out(out_seg, n_seg, "out_seg", dev)
    v, cnt = _results(results, _SEGMENT_OUTS, (n, n), dev)
    lib = _lib.load()
    _lib.check("pico_tcp_segment_batch_dev",
               lib.pico_tcp_segment_batch_dev(_ptr(base), base.numel(), _ptr(stream_desc), n, _ptr(groups), n_seg,
                                              _ptr(out), out.numel(), _ptr(out_desc), seg_stride, _ptr(out_seg),
                                              _ptr(cnt), _ptr(v), flags, _stream_handle(stream)))
    return v, cnt


_COALESCE_OUTS = (("verdict", torch.uint8, 1, True), ("out_len", torch.int32, 4, True), ("seg_verdict", torch.uint8, 1, True))


def tcp_coalesce_batch(base: torch.Tensor, seg_desc: torch.Tensor, n_seg: int, groups: torch.Tensor,
                       conn: torch.Tensor, out: torch.Tensor, out_desc: torch.Tensor, flags: int = 0, stream=None,
                       results=None):
    """TCP receive coalescing: every received segment verified and each connection's in-order byte
    stream delivered into one contiguous region in the same pass (pico_transport_crc_check,
    pico_socket.c:1916-1968; tcp_data_in, pico_tcp.c:1717-1776; pico_tcp_read, :1149-1182): the
    inverse of tcp_segment_batch, whose `out` / `out_seg` go in as `base` / `seg_desc`.  seg_desc = one
    received frame per descriptor (off -> IPv4 or IPv6 header, len = bytes available); groups = uint32
    (first segment, count) pairs per connection in arrival order, conn = uint32 (rcv_nxt, cflags) pairs
    (bit 0: sack_ok), both int32 tensors of 2*n; out = uint8 device buffer, out_desc[g] = the
    connection's region (off, capacity = the window).  flags: reserved, 0.  Returns (verdict uint8[n],
    out_len int32[n], seg_verdict uint8[n_seg]): V_ACCEPT / V_MALFORMED per connection, the stream
    bytes delivered (the new rcv_nxt is rcv_nxt + out_len), and per segment V_ACCEPT, V_NET_BAD,
    V_L4_BAD, V_MALFORMED, V_FRAG, V_TCP_CTRL, V_TCP_OLD or V_TCP_HELD; `results` may pass that triple
    preallocated, any of them None to skip it."""
    dev = _on_batch_device(base, seg_desc=seg_desc, groups=groups, conn=conn, out=out, out_desc=out_desc)
    _require_u8(base, "base")
    _require_u8(out, "out")
    n = _pairs(groups, "groups")
    _pairs(conn, "conn", n)
    _desc_bytes(seg_desc, n_seg, "seg_desc")
    _desc_bytes(out_desc, n, "out_desc")
    v, ol, sv = _results(results, _COALESCE_OUTS, (n, n, n_seg), dev)
    lib = _lib.load()
    _lib.check("pico_tcp_coalesce_batch_dev",
               lib.pico_tcp_coalesce_batch_dev(_ptr(base), base.numel(), _ptr(seg_desc), n_seg, _ptr(groups), _ptr(conn), n,
                                               _ptr(out), out.numel(), _ptr(out_desc), _ptr(ol), _ptr(sv), _ptr(v), flags,
                                               _stream_handle(stream)))
    return v, ol, sv


# struct pico_csum_tcp_ack (include/pico_csum.h): the ACK batch's per-connection record
TCP_ACK_DTYPE = np.dtype([("space", "<u4"), ("tsval", "<u4"), ("tsecr", "<u4"), ("aflags", "<u4")])
assert TCP_ACK_DTYPE.itemsize == 16
_ACK_OUTS = (("verdict", torch.uint8, 1, True), ("out_ack", torch.uint8, 1, True))


def tcp_ack_batch(base: torch.Tensor, seg_desc: torch.Tensor, n_seg: int, groups: torch.Tensor, conn: torch.Tensor,
                  out_len: torch.Tensor, seg_verdict: torch.Tensor, tmpl_base: torch.Tensor, tmpl_desc: torch.Tensor,
                  ack: torch.Tensor, out: torch.Tensor, out_desc: torch.Tensor, flags: int = 0, stream=None,
                  results=None):
    """The burst's ACKs, one launch behind tcp_coalesce_batch (tcp_send_ack -> tcp_send_empty,
    pico_tcp.c:1286-1327; tcp_sack_prepare, :1597-1657; tcp_add_options, :582-617; tcp_set_space,
    :681-700): base / seg_desc / n_seg / groups / conn as the coalescing took them, out_len (int32[n]) and
    seg_verdict (uint8[n_seg]) as it wrote them.  Every TCP_OLD / TCP_HELD segment's checksum is
    verified (seg_verdict is updated in place: such a segment may become V_L4_BAD, nothing else
    changes), and each connection with an ACCEPT, TCP_OLD or TCP_HELD segment gets one ACK frame at
    out_desc[g].off in `out`: ack = rcv_nxt + out_len, the window from ack[g].space, the options (WS,
    timestamps with aflags bit 0, the SACK blocks of the verified held segments with sack_ok) and both
    checksums.  tmpl_desc[g] -> the connection's network + 20-byte TCP header template in tmpl_base;
    ack = TCP_ACK_DTYPE records (uint8 / int32 tensor of 16 bytes a connection).  flags: reserved, 0.
    Returns (verdict uint8[n], out_ack uint8[16 n] = the frames' descriptors, {0, 0, 0} where no ACK is
    due); `results` may pass that pair preallocated, either of them None to skip it."""
    dev = _on_batch_device(base, seg_desc=seg_desc, groups=groups, conn=conn, out_len=out_len, seg_verdict=seg_verdict,
                           tmpl_base=tmpl_base, tmpl_desc=tmpl_desc, ack=ack, out=out, out_desc=out_desc)
    _require_u8(base, "base")
    _require_u8(tmpl_base, "tmpl_base")
    _require_u8(out, "out")
    n = _pairs(groups, "groups")
    _pairs(conn, "conn", n)
    _desc_bytes(seg_desc, n_seg, "seg_desc")
    _desc_bytes(tmpl_desc, n, "tmpl_desc")
    _desc_bytes(out_desc, n, "out_desc")
    _desc_bytes(ack, n, "ack")
    if not ack.is_contiguous():
        raise ValueError("ack must be a contiguous tensor of 16-byte records")
    _check_out(out_len, n, "out_len", dev, 4)
    _check_out(seg_verdict, n_seg, "seg_verdict", dev, 1)
    v, oa = _results(results, _ACK_OUTS, (n, 16 * n), dev)
    lib = _lib.load()
    _lib.check("pico_tcp_ack_batch_dev",
               lib.pico_tcp_ack_batch_dev(_ptr(base), base.numel(), _ptr(seg_desc), n_seg, _ptr(groups), _ptr(conn), n,
                                          _ptr(out_len), _ptr(seg_verdict), _ptr(tmpl_base), tmpl_base.numel(),
                                          _ptr(tmpl_desc), _ptr(ack), _ptr(out), out.numel(), _ptr(out_desc), _ptr(oa),
                                          _ptr(v), flags, _stream_handle(stream)))
    return v, oa


# struct pico_csum_icmp4_req / pico_csum_icmp4_state (include/pico_csum.h): the ICMPv4 answers' per-record
# request and the carried duplicate state
ICMP4_REQ_DTYPE = np.dtype([("src", "<u4"), ("id", "<u2"), ("type", "u1"), ("code", "u1")])
ICMP4_STATE_DTYPE = np.dtype([("seen", "<u4"), ("id", "<u2"), ("seq", "<u2")])
assert ICMP4_REQ_DTYPE.itemsize == 8 and ICMP4_STATE_DTYPE.itemsize == 8
_ICMP4_OUTS = (("verdict", torch.uint8, 1, False), ("out_ans", torch.uint8, 1, True))


def icmp4_state(device) -> torch.Tensor:
    """An echo duplicate state (struct pico_csum_icmp4_state) at the reference's initial value (firstpkt:
    seen = 0)."""
    return torch.zeros(ICMP4_STATE_DTYPE.itemsize, dtype=torch.uint8, device=device)


def icmp4_reply_batch(base: torch.Tensor, desc: torch.Tensor, n: int, req: torch.Tensor, out: torch.Tensor,
                      out_desc: torch.Tensor, *, state: torch.Tensor | None, flags: int = 0, stream=None, results=None):
    """A burst's ICMPv4 answers (pico_icmp4_process_in, pico_icmp4.c:47-85, with pico_icmp4_checksum :30-41
    and pico_ipv4_rebound / pico_ipv4_frame_push, pico_ipv4.c:1512-1533, :1039-1079; pico_icmp4_notify,
    pico_icmp4.c:106-141): desc = one answered datagram per descriptor (off -> its IPv4 header, len = bytes
    available), req = ICMP4_REQ_DTYPE records (uint8 / int32 tensor of 8 bytes a record: the answer's source
    as stored, its IPv4 id, type 0 = echo reply to an echo request, 3 / 11 / 12 + code = that notice), out =
    uint8 device buffer, out_desc[i] = the answer's region (off, capacity).  `state` (icmp4_state()) carries
    the last echo request's (id, seq) from one call to the next, as the reference's statics do; state=None
    is the explicit one-shot mode (nothing carried, nothing kept).  flags: reserved, 0.  Returns (verdict
    uint8[n]: V_ACCEPT, V_UNTOUCHED, V_DUPLICATE or V_MALFORMED; out_ans uint8[16 n] = the answers'
    descriptors, {0, 0, 0} where none was written); `results` may pass that pair preallocated, out_ans None
    to skip it."""
    tensors = dict(desc=desc, req=req, out=out, out_desc=out_desc)
    if state is not None:
        tensors["state"] = state
    dev = _on_batch_device(base, **tensors)
    _require_u8(base, "base")
    _require_u8(out, "out")
    if n < 0:
        raise ValueError(f"n = {n}")
    _desc_bytes(desc, n, "desc")
    _desc_bytes(out_desc, n, "out_desc")
    if not req.is_contiguous() or req.numel() * req.element_size() < 8 * n:
        raise ValueError(f"req must be a contiguous tensor of {n} 8-byte records")
    if state is not None and (not state.is_contiguous() or state.numel() * state.element_size() < 8):
        raise ValueError("state must be a contiguous 8-byte tensor (icmp4_state())")
    if results is not None and results[0] is None:
        raise ValueError("verdict is required: the launches hand their work on through it")
    v, oa = _results(results, _ICMP4_OUTS, (n, 16 * n), dev)
    lib = _lib.load()
    _lib.check("pico_icmp4_reply_batch_dev",
               lib.pico_icmp4_reply_batch_dev(_ptr(base), base.numel(), _ptr(desc), n, _ptr(req), _ptr(state), _ptr(out),
                                              out.numel(), _ptr(out_desc), _ptr(oa), _ptr(v), flags, _stream_handle(stream)))
    return v, oa


# struct pico_csum_icmp6_req (include/pico_csum.h): the ICMPv6 answers' per-record request
ICMP6_REQ_DTYPE = np.dtype([("src", "u1", 16), ("arg", "<u4"), ("type", "u1"), ("code", "u1"), ("hop", "u1"), ("rsvd", "u1")])
assert ICMP6_REQ_DTYPE.itemsize == 24


def icmp6_reply_batch(base: torch.Tensor, desc: torch.Tensor, n: int, req: torch.Tensor, out: torch.Tensor,
                      out_desc: torch.Tensor, flags: int = 0, stream=None, results=None):
    """A burst's ICMPv6 answers (pico_icmp6_process_in / pico_icmp6_send_echoreply, pico_icmp6.c:94-133, :61-92,
    with pico_icmp6_checksum :38-55 and pico_ipv6_frame_push, pico_ipv6.c:1324-1339; pico_icmp6_notify,
    pico_icmp6.c:153-227): desc = one answered datagram per descriptor (off -> its IPv6 header, len = bytes
    available), req = ICMP6_REQ_DTYPE records (uint8 / int32 tensor of 24 bytes a record: the answer's source,
    type 4's pointer / type 2's MTU, type 0 = echo reply to an echo request, 1 / 2 / 3 / 4 + code = that
    notice, the hop limit), out = uint8 device buffer, out_desc[i] = the answer's region (off, capacity).
    There is no state: the reference keeps none for ICMPv6, repeats are answered.  flags: reserved, 0.
    Returns (verdict uint8[n]: V_ACCEPT, V_UNTOUCHED or V_MALFORMED; out_ans uint8[16 n] = the answers'
    descriptors, {0, 0, 0} where none was written); `results` may pass that pair preallocated, out_ans None
    to skip it."""
    dev = _on_batch_device(base, desc=desc, req=req, out=out, out_desc=out_desc)
    _require_u8(base, "base")
    _require_u8(out, "out")
    if n < 0:
        raise ValueError(f"n = {n}")
    _desc_bytes(desc, n, "desc")
    _desc_bytes(out_desc, n, "out_desc")
    if not req.is_contiguous() or req.numel() * req.element_size() < 24 * n:
        raise ValueError(f"req must be a contiguous tensor of {n} 24-byte records")
    if flags != 0:
        raise ValueError(f"flags = {flags:#x}: none is defined for this batch")
    if results is not None and results[0] is None:
        raise ValueError("verdict is required: the launches hand their work on through it")
    v, oa = _results(results, _ICMP4_OUTS, (n, 16 * n), dev)
    # the library's alignment rules (a view into a larger tensor may break them), stated before it is reached
    for name, t, align in (("desc", desc, 16), ("out_desc", out_desc, 16), ("out_ans", oa, 16), ("req", req, 4)):
        if t is not None and t.data_ptr() % align:
            raise ValueError(f"{name} must be {align}-byte aligned")
    lib = _lib.load()
    _lib.check("pico_icmp6_reply_batch_dev",
               lib.pico_icmp6_reply_batch_dev(_ptr(base), base.numel(), _ptr(desc), n, _ptr(req), _ptr(out), out.numel(),
                                              _ptr(out_desc), _ptr(oa), _ptr(v), flags, _stream_handle(stream)))
    return v, oa


icmp6_reply = icmp6_reply_batch


# struct pico_csum_flow_key (include/pico_csum.h): one entry of the flow grouping's connection table
FLOW_KEY_DTYPE = np.dtype([("src", "u1", 16), ("dst", "u1", 16), ("sport", "<u2"), ("dport", "<u2"), ("family", "u1"),
                           ("reserved", "u1", 3)])
assert FLOW_KEY_DTYPE.itemsize == 40
_FLOW_OUTS = (("out_desc", torch.uint8, 1, False), ("out_index", torch.int32, 4, False), ("out_groups", torch.int32, 4, False),
              ("out_counts", torch.int32, 4, False))


def flow_group_scratch_bytes(n: int, n_known: int = 0) -> int:
    """pico_flow_group_scratch_bytes: the scratch a grouping of n frames against n_known table keys needs
    (host arithmetic; 0 = out of range)."""
    if not (0 <= n <= 0xFFFFFFFF and 0 <= n_known <= 0xFFFFFFFF):
        return 0
    return int(_lib.load().pico_flow_group_scratch_bytes(n, n_known))


def flow_group_batch(base: torch.Tensor, desc: torch.Tensor, n: int, mode_flags: int, verdict_in: torch.Tensor | None = None,
                     known: torch.Tensor | None = None, n_known: int = 0, hash_seed: int = 0,
                     scratch: torch.Tensor | None = None, stream=None, results=None):
    """Flow grouping (pico_flow_group_batch_dev; the batch form of pico_socket_tcp_deliver's and the
    fragment trees' key comparisons): the n frames of a verified burst, in arrival order, become the
    group-contiguous descriptors and the (first, count) groups that ipv4_reassemble_batch,
    ipv6_reassemble_batch and tcp_coalesce_batch take.  mode_flags = FLOW_TCP / FLOW_FRAG4 / FLOW_FRAG6,
    | FLOW_F_ETH when desc.off -> the Ethernet header; verdict_in = the RX batch's verdicts (uint8[n]) or
    None; known = the connection table (uint8 tensor of 40 * n_known bytes, FLOW_KEY_DTYPE; TCP mode),
    whose keys own groups 0 .. n_known-1; scratch = a uint8 tensor of flow_group_scratch_bytes(n, n_known)
    bytes (None allocates one).  Returns (out_desc uint8[16 n], out_index int32[n], out_groups
    int32[2 (n + n_known)], out_counts int32[2] = n_groups, selected frames); `results` may pass that
    quadruple preallocated."""
    tensors = dict(desc=desc)
    for name, t in (("verdict_in", verdict_in), ("known", known), ("scratch", scratch)):
        if t is not None:
            tensors[name] = t
    dev = _on_batch_device(base, **tensors)
    _require_u8(base, "base")
    if n <= 0 or n_known < 0:
        raise ValueError(f"n = {n}, n_known = {n_known}: at least one frame")
    need = flow_group_scratch_bytes(n, n_known)
    if need == 0:
        raise ValueError(f"n + n_known = {n + n_known} is out of range (at most 0x00FFFFFF)")
    _desc_bytes(desc, n, "desc")
    if verdict_in is not None:
        _check_out(verdict_in, n, "verdict_in", dev, 1)
    if n_known:
        if known is None or not known.is_contiguous() or known.numel() * known.element_size() < 40 * n_known:
            raise ValueError(f"known must be a contiguous tensor of {n_known} 40-byte keys")
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    _require_u8(scratch, "scratch")
    if scratch.numel() < need:
        raise ValueError(f"scratch holds {scratch.numel()} bytes, the batch needs {need}")
    od, oi, og, oc = _results(results, _FLOW_OUTS, (16 * n, n, 2 * (n + n_known), 2), dev)
    lib = _lib.load()
    _lib.check("pico_flow_group_batch_dev",
               lib.pico_flow_group_batch_dev(_ptr(base), base.numel(), _ptr(desc), n, _ptr(verdict_in), mode_flags,
                                             _ptr(known) if n_known else None, n_known, hash_seed & 0xFFFFFFFF, _ptr(od),
                                             _ptr(oi), _ptr(og), _ptr(oc), _ptr(scratch), scratch.numel(),
                                             _stream_handle(stream)))
    return od, oi, og, oc


STREAM_OFF = 0xFF


def set_uniform_stream(mode: int = 0, frames_per_wave: int = 0) -> None:
    """Uniform rings' stream waves (tests / bench sweeps, this thread): mode 0 automatic, 1 on where
    the ring allows them, STREAM_OFF the lane-group kernels; frames per wave (0 = automatic).
    Results never depend on it (include/pico_csum.h)."""
    _lib.check("pico_csum_set_uniform_stream", _lib.load().pico_csum_set_uniform_stream(mode, frames_per_wave))


def set_host_in_place(on: bool = True) -> None:
    """Host-resident descriptor batches (this thread): read a device-addressable (page-locked) burst
    in place (True, the default) or always stage it (False).  Results never depend on it."""
    _lib.check("pico_csum_set_host_in_place", _lib.load().pico_csum_set_host_in_place(1 if on else 0))


def set_reasm_flat(mode: int = 0) -> None:
    """Reassembly batches' flat grid (tests / bench sweeps, this thread): 0 automatic (batches from
    512 datagrams), 1 always, 2 never.  Results never depend on it."""
    _lib.check("pico_csum_set_reasm_flat", _lib.load().pico_csum_set_reasm_flat(mode))


def set_launch_override(group: int = 0, cpl: int = 0, fpw: int = 0, unroll: int | None = None, nt: int = 0,
                        pipeline: int = 0) -> None:
    """Force a kernel launch shape (tests / bench sweeps): group 0 = automatic; 2 = descriptor
    batches with `fpw` frames per wave; 4..64 = uniform rings (lanes per frame, cpl, fpw,
    unroll, nt, pipeline as in include/pico_csum.h)."""
    if unroll is None:
        unroll = 0 if group == 2 else 1
    if group in (0, 2):
        unroll = cpl = nt = pipeline = 0
        if group == 0:
            fpw = 0
    _lib.check("pico_csum_set_launch_override",
               _lib.load().pico_csum_set_launch_override(group, cpl, unroll, fpw, nt, pipeline))


class HostBatch:
    """Host-resident batches (pico_checksum_batch_uniform_host and the descriptor batches
    pico_{checksum,ipv4_checksum,ipv6_checksum,eth_checksum}_batch_host): H2D, kernel and
    D2H chunked over two streams (staging_bytes per chunk)."""

    def __init__(self, device: int = 0, staging_bytes: int = 64 << 20):
        self._lib = _lib.load()
        self._ctx = self._lib.pico_csum_ctx_create(device, staging_bytes)
        if not self._ctx:
            raise _lib.PicoCsumError("pico_csum_ctx_create", -1,
                                     self._lib.pico_csum_last_error().decode(errors="replace"))

    def checksum_uniform(self, frames: np.ndarray | torch.Tensor, stride: int, length: int, n: int,
                         seed: int = 0, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.empty(n, dtype=np.uint16)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint16 and out.flags.c_contiguous
                and out.size >= n):
            raise ValueError("out must be a contiguous uint16 array of at least n elements")
        need = (n - 1) * stride + length if n else 0
        if isinstance(frames, torch.Tensor):
            if frames.is_cuda:
                raise ValueError("HostBatch takes host memory")
            if not frames.is_contiguous():
                raise ValueError("frames must be contiguous")
            nbytes = frames.numel() * frames.element_size()
            src = frames.data_ptr()
        else:
            if not frames.flags.c_contiguous:
                raise ValueError("frames must be contiguous")
            nbytes = frames.nbytes
            src = frames.ctypes.data
        if nbytes < need:
            raise ValueError(f"frames hold {nbytes} bytes, the batch spans {need}")
        _lib.check("pico_checksum_batch_uniform_host",
                   self._lib.pico_checksum_batch_uniform_host(self._ctx, ctypes.c_void_p(src), stride, length, n,
                                                              seed & 0xFFFFFFFF,
                                                              ctypes.c_void_p(out.ctypes.data)))
        return out

    @staticmethod
    def _host(a: np.ndarray, name: str, dtype=None) -> int:
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous or (dtype is not None and a.dtype != dtype):
            raise ValueError(f"{name} must be a contiguous numpy array" + (f" of {dtype}" if dtype else ""))
        return a.ctypes.data

    def _desc_args(self, base: np.ndarray, desc: np.ndarray):
        if not (isinstance(base, np.ndarray) and base.dtype == np.uint8 and base.flags.c_contiguous):
            raise ValueError("base must be a contiguous uint8 numpy array (host memory)")
        d = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        return d, ctypes.c_void_p(base.ctypes.data), base.size, ctypes.c_void_p(d.ctypes.data), d.size

    def _outs(self, n, *spec):
        return [np.zeros(n, dtype=dt) for dt in spec]

    def checksum_batch(self, base: np.ndarray, desc: np.ndarray, crc_off: int = -1, flags: int = 0) -> np.ndarray:
        """pico_checksum_batch_host: raw descriptor batch from host memory (F_WRITE stores in `base`)."""
        d, b, bl, dp, n = self._desc_args(base, desc)
        (out,) = self._outs(n, np.uint16)
        _lib.check("pico_checksum_batch_host",
                   self._lib.pico_checksum_batch_host(self._ctx, b, bl, dp, n, crc_off, flags,
                                                      ctypes.c_void_p(out.ctypes.data)))
        return out

    def ipv4_checksum_batch(self, base: np.ndarray, desc: np.ndarray, flags: int = 0, out=None):
        """`out` may pass the (out_net uint16, out_transport uint16, verdict uint8) host arrays -- e.g.
        page-locked ones, which with a page-locked burst and descriptors make the call zero-copy."""
        d, b, bl, dp, n = self._desc_args(base, desc)
        if out is None:
            on, ol, v = self._outs(n, np.uint16, np.uint16, np.uint8)
        else:
            on, ol, v = out
            for a, nm, dt in ((on, "out_net", np.uint16), (ol, "out_transport", np.uint16), (v, "verdict", np.uint8)):
                self._host(a, nm, dt)
                if a.size < n:
                    raise ValueError(f"{nm} shorter than n")
        _lib.check("pico_ipv4_checksum_batch_host",
                   self._lib.pico_ipv4_checksum_batch_host(self._ctx, b, bl, dp, n, flags, on.ctypes.data,
                                                           ol.ctypes.data, v.ctypes.data))
        return on, ol, v

    def ipv6_checksum_batch(self, base: np.ndarray, desc: np.ndarray, flags: int = 0):
        d, b, bl, dp, n = self._desc_args(base, desc)
        ol, v = self._outs(n, np.uint16, np.uint8)
        _lib.check("pico_ipv6_checksum_batch_host",
                   self._lib.pico_ipv6_checksum_batch_host(self._ctx, b, bl, dp, n, flags, ol.ctypes.data,
                                                           v.ctypes.data))
        return ol, v

    def eth_checksum_batch(self, base: np.ndarray, desc: np.ndarray, flags: int = 0, mac: bytes | None = None):
        d, b, bl, dp, n = self._desc_args(base, desc)
        on, ol, v = self._outs(n, np.uint16, np.uint16, np.uint8)
        m = None if mac is None else ctypes.create_string_buffer(bytes(mac), 6)
        _lib.check("pico_eth_checksum_batch_host",
                   self._lib.pico_eth_checksum_batch_host(self._ctx, b, bl, dp, n, flags, m, on.ctypes.data,
                                                          ol.ctypes.data, v.ctypes.data))
        return on, ol, v

    def close(self) -> None:
        if self._ctx:
            self._lib.pico_csum_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
