/*
 * pico_csum.h -- C ABI of libpicocsum, the MI355X-native drop-in for picoTCP's
 * Internet-checksum path (RFC 1071 one's-complement sum, stack/pico_frame.c).
 *
 * Plain C: no torch, no HIP types in any signature.  Device pointers are
 * plain `void *` / `T *`; a HIP stream is passed as an opaque `void *`
 * (NULL = the device's default stream).
 *
 * Three layers:
 *
 *  1. Scalar drop-in (replaces the two strong symbols of the reference's
 *     stack/pico_frame.o; callers keep compiling against
 *     include/pico_frame.h unchanged):
 *       pico_checksum            ref: include/pico_frame.h:106, stack/pico_frame.c:312-318
 *       pico_dualbuffer_checksum ref: include/pico_frame.h:107, stack/pico_frame.c:320-328
 *     The reference calls these inline, once per frame, from a single-threaded
 *     tick loop on host pointers.  A GPU launch costs ~10 us
 *     against ~100 ns of work, so these two stay synchronous host code with
 *     bit-identical results; the accelerated path is layer 2.
 *
 *  2. Batched device API (the MI355X hot path; the reference has no batch
 *     entry -- each function below is the batch form of the per-frame calls
 *     cited on it).  Buffers are device-resident; calls are asynchronous on
 *     `stream`; they never fall back to host code: when no HIP device or
 *     kernel image is usable they return -PICO_ERR_ENODEV and set
 *     pico_csum_last_error().
 *
 *  3. Host-resident batch API: H2D -> kernel -> D2H, chunked and overlapped on
 *     two streams (the path starts and ends in host memory: a pico_device /
 *     TAP buffer, modules/pico_dev_tap.c:53-79).
 *
 * Return convention of every checksum value (device and host alike) is the
 * reference's: ret = short_be((uint16_t)~fold(sum)); a caller stores
 * hdr->crc = short_be(ret), and a region that already carries its correct
 * checksum yields 0 (pico_ipv4.c:249, pico_socket.c:1927).
 *
 * Error codes: 0 on success, otherwise the negated picoTCP pico_err value
 * (include/pico_protocol.h:21-65).
 */
#ifndef PICO_CSUM_H
#define PICO_CSUM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (a caller must check pico_csum_abi_version() == PICO_CSUM_ABI_VERSION):
 *   2: V_FRAG, the reference's IPv6 byte-9 dispatch by default;
 *   3: F_NXTHDR_DISPATCH moved to 0x8 (bit 0x4 -- ABI 1's F_REF_DISPATCH, the opposite meaning --
 *      is rejected with -EINVAL); the forwarding batch takes the host's link addresses and a
 *      carried state (pico_ipv4_pre_forward_checks in full);
 *   4: pico_csum_release_thread_scratch; the reassembly's flat-grid scratch is freed at thread exit;
 *   4 (added, no bump): pico_ipv4_fragment_batch_dev -- a new entry point breaks no caller;
 *   4 (added, no bump): pico_tcp_segment_batch_dev -- likewise;
 *   4 (added, no bump): pico_tcp_coalesce_batch_dev and its three verdict values, which no other batch
 *      returns -- likewise;
 *   4 (added, no bump): pico_flow_group_batch_dev, pico_flow_group_scratch_bytes, struct pico_csum_flow_key
 *      and the PICO_CSUM_FLOW_* modes -- likewise;
 *   4 (added, no bump): pico_tcp_ack_batch_dev and struct pico_csum_tcp_ack -- likewise;
 *   4 (added, no bump): pico_icmp4_reply_batch_dev, struct pico_csum_icmp4_req and struct
 *      pico_csum_icmp4_state -- likewise;
 *   4 (added, no bump): pico_icmp6_reply_batch_dev and struct pico_csum_icmp6_req -- likewise;
 *   4 (added, no bump): pico_ipv6_fragment_batch_dev -- likewise. */
#define PICO_CSUM_ABI_VERSION 4

/* picoTCP pico_err values used here (include/pico_protocol.h:27,31,38 + ENODEV) */
#define PICO_CSUM_EIO     5
#define PICO_CSUM_ENOMEM 12
#define PICO_CSUM_EINVAL 22
#define PICO_CSUM_ENODEV 19

/* One frame region of a batch: 16 bytes, naturally aligned. */
#ifndef PICO_CSUM_DESC_DEFINED
#define PICO_CSUM_DESC_DEFINED
struct pico_csum_desc {
    uint64_t off;   /* byte offset of the region from the batch base (any alignment) */
    uint32_t len;   /* RAW: region length (the `len` of pico_checksum);
                       IPV4: bytes available from the IPv4 header to the end of
                       the frame buffer = f->buffer_len - (f->net_hdr - f->buffer) */
    uint32_t seed;  /* RAW: initial pico_checksum_adder accumulator, e.g. a
                       pseudo-header partial from pico_ipv4_pseudo_partial()
                       (TX: from socket state, pico_tcp.c:429-433); 0 for a
                       plain pico_checksum.  IPV4: must be 0 (reserved). */
};
#endif

/* flags */
#define PICO_CSUM_F_WRITE 0x1u  /* store short_be(ret) into the frame's crc field (in place, device memory) */
#define PICO_CSUM_F_TX    0x2u  /* fused batches: compute (TX) mode -- crc fields read as zero */
/* IPv6 / Ethernet batches, RX.  By default the IPv6 TCP / UDP transport check is dispatched
 * exactly as the reference's pico_transport_crc_check does it (stack/pico_socket.c:1919-1923):
 * on `proto` read through a struct pico_ipv4_hdr cast of the network header -- for IPv6 that is
 * byte 9, the source address's second byte: 6 -> pico_tcp_checksum (TCP pseudo header), 17 ->
 * the UDP check when transport bytes 6-7 are non-zero (UDP pseudo header), anything else -> no
 * check.  With this flag the check follows the transport's own protocol instead (TCP always,
 * UDP when its crc != 0: the evident intent, not the reference's behaviour).  ICMPv6 is the
 * same either way (pico_icmp6_process_in checks it itself). */
#define PICO_CSUM_F_NXTHDR_DISPATCH 0x8u
#define PICO_CSUM_F_RETIRED_0x4     0x4u  /* ABI 1's F_REF_DISPATCH: rejected (-EINVAL) since ABI 3 */

/* Verdict byte of the fused batches: the reference's FIRST outcome for the frame, in its own
 * order (one value, plus V_IPV6 on the Ethernet batch's IPv6 frames).
 * The values are per batch kind: bits 16, 32 and 64 mean different things in different batches
 * (V_FRAG / V_EXPIRED; V_DROP_L2 / V_UNTOUCHED / V_LOCAL_SRC; V_ARP / V_DUPLICATE).  Decode a
 * verdict array only with the list given at the batch that produced it:
 *   RX / TX (IPv4, IPv6):  ACCEPT, NET_BAD (IPv4), L4_BAD, MALFORMED, FRAG
 *   Ethernet:              the RX / TX list, DROP_L2, ARP, | IPV6
 *   forwarding:            ACCEPT, MALFORMED, EXPIRED, LOCAL_SRC, DUPLICATE
 *   NAT:                   ACCEPT, MALFORMED, FRAG, UNTOUCHED
 *   reassembly:            ACCEPT, L4_BAD, MALFORMED
 *   fragmentation (TX):    ACCEPT, MALFORMED
 *   TCP segmentation (TX): ACCEPT, MALFORMED
 *   TCP coalescing (RX):   per connection ACCEPT, MALFORMED; per segment ACCEPT, NET_BAD (IPv4), L4_BAD,
 *                          MALFORMED, FRAG, TCP_CTRL, TCP_OLD, TCP_HELD */
#define PICO_CSUM_V_ACCEPT    1u  /* delivered to the transport and every checksum the reference
                                     checks passes: hand the frame on (a stack built with CRC=0
                                     need not check it again) */
#define PICO_CSUM_V_NET_BAD   2u  /* pico_ipv4_crc_check discards it (pico_ipv4.c:420-422, :243-257) */
#define PICO_CSUM_V_L4_BAD    4u  /* pico_transport_crc_check discards it (pico_socket.c:1929,1953) */
#define PICO_CSUM_V_MALFORMED 8u  /* discarded before any transport: infeasible length
                                     (pico_ipv4.c:405-408); after a good header checksum an invalid
                                     source (:425-428), the evil bit (:431-435), IHL < 5 (:438-443);
                                     an IPv6 extension-header chain pico_ipv6_extension_headers
                                     discards (pico_ipv6.c:659-809); a header or field that lies
                                     past the buffer (where the reference would read past it) */
#define PICO_CSUM_V_FRAG     16u  /* a fragment: IPv4 MF or offset (pico_ipv4.c:446-455), IPv6 a
                                     fragment header (pico_ipv6.c:791-795) -- header verified, NO
                                     transport check (the reference checks the reassembled
                                     datagram): route it to the reassembly batch.  TX: the
                                     header checksum only (the transport's covers the datagram). */
#define PICO_CSUM_V_EXPIRED  16u  /* forwarding batch only (same bit): TTL reached 0 (pico_ipv4.c:1549-1552) */
#define PICO_CSUM_V_LOCAL_SRC 32u /* forwarding batch only: the source is one of the host's link addresses
                                     (pico_ipv4.c:1559-1560) */
#define PICO_CSUM_V_DUPLICATE 64u /* forwarding batch only: (src, id, dst, proto) of the last forwarded
                                     datagram (pico_ipv4.c:1562-1565) */
#define PICO_CSUM_V_DROP_L2  32u  /* Ethernet batch: discarded by the link layer -- foreign destination MAC
                                     (pico_ethernet.c:221-231), unknown ethertype (:201-202) or an IP
                                     version that does not match it (:143-150, :162-176) */
#define PICO_CSUM_V_ARP      64u  /* Ethernet batch: ARP frame, handed to pico_arp_receive (:186-187) */
#define PICO_CSUM_V_IPV6    128u  /* Ethernet batch: set on every IPv6 frame (ethertype 0x86DD) */
#define PICO_CSUM_V_UNTOUCHED 32u /* NAT batch only (same bit as V_DROP_L2): left as it is -- no
                                     rewrite record (the host's tuple lookup failed), or a protocol
                                     the reference's NAT returns -1 on (pico_nat.c:472-474, :537-539) */

#define PICO_CSUM_V_TCP_CTRL  32u /* TCP coalescing batch only (same bit as V_DROP_L2): a segment for the host's
                                     state machine -- flags other than ACK or PSH|ACK (SYN, FIN, RST, none:
                                     tcp_action_by_flags, pico_tcp.c:2787-2815) or no payload
                                     (segment_from_frame returns NULL, :101); header verified, NO transport check */
#define PICO_CSUM_V_TCP_OLD   64u /* TCP coalescing batch only (same bit as V_ARP): not on the chain, seq before
                                     its end -- a duplicate, a retransmission or an overlap, which the reference
                                     drops (pico_tcp.c:1687); payload not read */
#define PICO_CSUM_V_TCP_HELD 128u /* TCP coalescing batch only (same bit as V_IPV6): not on the chain, seq at or
                                     beyond its end -- not delivered in this call; payload not read */

/* ---------------------------------------------------------------- layer 1 */

/* ref: stack/pico_frame.c:312-318 */
uint16_t pico_checksum(void *inbuf, uint32_t len);
/* ref: stack/pico_frame.c:320-328 (len1 must be even, as in the reference) */
uint16_t pico_dualbuffer_checksum(void *inbuf1, uint32_t len1, void *inbuf2, uint32_t len2);

/* The reference's accumulator step, exported so a caller can build a
 * descriptor seed: ref stack/pico_frame.c:279-299 pico_checksum_adder. */
uint32_t pico_checksum_partial(uint32_t sum, const void *buf, uint32_t len);
/* Accumulator value of the 12-byte struct pico_ipv4_pseudo_hdr
 * (modules/pico_ipv4.h:46-53) as pico_tcp_checksum_ipv4 / pico_udp_checksum_ipv4
 * build it (pico_tcp.c:428-443, pico_udp.c:42-57).  src/dst as stored in
 * struct pico_ip4 (network byte order). */
uint32_t pico_ipv4_pseudo_partial(uint32_t src_addr, uint32_t dst_addr, uint8_t proto, uint16_t transport_len);
/* Accumulator value of the 40-byte struct pico_ipv6_pseudo_hdr (modules/pico_ipv6.h:46-53:
 * src, dst, long_be(len), 3 zero bytes, nxthdr) as pico_tcp_checksum_ipv6 /
 * pico_udp_checksum_ipv6 / pico_icmp6_checksum / pico_mld_checksum build it
 * (pico_tcp.c:449-475, pico_udp.c:63-92, pico_icmp6.c:38-55, pico_mld.c:421-437).
 * A raw batch seeded with it serves the MLD router-alert variant (transport + 8,
 * length - 8) and TX datagrams whose addresses come from the socket. */
uint32_t pico_ipv6_pseudo_partial(const void *src16, const void *dst16, uint8_t nxthdr, uint32_t transport_len);

/* ---------------------------------------------------------------- layer 2 */

/* Every device batch takes the size of the buffer behind d_base (base_len).
 * Nothing outside [d_base, d_base + base_len) is ever written, and no byte outside it
 * contributes to a result.  The kernels load whole 16-byte-aligned blocks, so the
 * 16-byte-aligned blocks that overlap [d_base, d_base + base_len) may be read in full
 * (up to 15 bytes before d_base and after its end; such a block never crosses a page,
 * so this cannot fault).  A caller that writes those neighbouring bytes from another
 * stream concurrently gets correct results all the same: they are masked out.
 *
 * Batch of pico_checksum / pico_dualbuffer_checksum calls:
 *   d_out[i] = finalize(adder(desc[i].seed, d_base + desc[i].off, desc[i].len))
 * crc_off >= 0 (even): the 2 bytes at off+crc_off read as zero when they lie
 * inside the region ("hdr->crc = 0" before computing: pico_ipv4.c:237,
 * pico_icmp4.c:38, pico_tcp.c:980); with PICO_CSUM_F_WRITE the result is
 * stored there (pico_ipv4.c:238, pico_icmp4.c:39, pico_tcp.c:981).
 * crc_off < 0: no crc field.  Regions may not overlap when F_WRITE is set.
 * A region that does not lie inside base_len is not read: d_out[i] = 0 and,
 * when d_bad != NULL, *d_bad (a device uint32 the caller zeroes) counts it. */
int pico_checksum_batch_dev(void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc,
                            uint32_t n, int32_t crc_off, uint32_t flags, uint16_t *d_out,
                            uint32_t *d_bad, void *stream);

/* Uniform batch (no descriptors): frame i = d_base + i*stride, len bytes,
 * seed added to every frame.  The layout of a packed frame ring.
 * (n-1)*stride + len must not exceed base_len (else -EINVAL). */
int pico_checksum_batch_uniform_dev(const void *d_base, uint64_t base_len, uint64_t stride, uint32_t len,
                                    uint32_t n, uint32_t seed, uint16_t *d_out, void *stream);

/* Fused IPv4 header + transport batch, one IPv4 datagram per descriptor
 * (desc.off -> IPv4 header, desc.len = bytes available).
 * RX (flags without F_TX): pico_ipv4_process_in (pico_ipv4.c:381-456) up to its hand-off --
 *   lengths, pico_ipv4_crc_check (:243-257), the source check, the evil bit, IHL < 5, the
 *   fragment hand-off -- then pico_transport_crc_check (pico_socket.c:1916-1968): TCP always,
 *   UDP when its crc field != 0, pseudo header from the IP header.  The link-directed
 *   broadcast sources of pico_ipv4_is_broadcast (the stack's link table) are left to the stack.
 *   d_out_net = pico_checksum(hdr, net_len), d_out_transport = the TCP/UDP
 *   checksum (0 = valid; 0 when none is computed), d_verdict = PICO_CSUM_V_*.
 * TX (F_TX): crc fields read as zero; d_out_* are the values to store
 *   (IPv4 header; TCP with pseudo header; ICMPv4 without; UDP 0 as
 *   pico_udp.c:123).  F_WRITE stores them into accepted frames in place.
 * A datagram whose [off, off+len) is not inside base_len is MALFORMED, unread.
 * Any output pointer may be NULL. */
int pico_ipv4_checksum_batch_dev(void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc,
                                 uint32_t n, uint32_t flags, uint16_t *d_out_net,
                                 uint16_t *d_out_transport, uint8_t *d_verdict, void *stream);

/* Fused IPv6 transport batch (TCP / UDP / ICMPv6 over IPv6),
 * one datagram per descriptor: desc.off -> IPv6 header, desc.len = bytes available,
 * desc.seed = 0, or f->net_len | (transport proto << 16) when the stack already walked the
 * extension headers.  RX with seed 0: the kernel walks them itself, as
 * pico_ipv6_extension_headers does (pico_ipv6.c:659-809: the sequence check, hop-by-hop /
 * routing / fragment / destination-option processing): a chain the reference discards is
 * V_MALFORMED, a transport behind a fragment header V_FRAG.  TX with seed 0: net_len 40,
 * proto = hdr->nxthdr.  transport_len = (uint16)(payload_len - (net_len - 40))
 * (pico_ipv6.c:790); pseudo header = struct pico_ipv6_pseudo_hdr (pico_ipv6.h:46-53) from
 * the IPv6 header.
 * RX: pico_transport_crc_check (pico_socket.c:1916-1968; pico_tcp_checksum_ipv6
 *   pico_tcp.c:449-475, pico_udp_checksum_ipv6 pico_udp.c:63-92) dispatched on header byte 9
 *   as the reference does (see PICO_CSUM_F_NXTHDR_DISPATCH for the alternative); ICMPv6
 *   (pico_icmp6_checksum pico_icmp6.c:38-55) is always computed, V_L4_BAD only for the ND /
 *   MLD types the reference checks (pico_ipv6_nd.c:595, pico_mld.c:415).
 * TX (F_TX): crc field read as zero (pico_tcp.c:980, pico_ipv6.c:1337,1345);
 *   F_WRITE stores it.  d_out_transport: the checksum (0 = valid on RX). */
int pico_ipv6_checksum_batch_dev(void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc,
                                 uint32_t n, uint32_t flags, uint16_t *d_out_transport, uint8_t *d_verdict,
                                 void *stream);

/* Ethernet front end of the fused RX verify, one frame per descriptor,
 * IPv4, IPv6, ARP and other ethertypes mixed in ONE launch: desc.off -> the Ethernet header
 * (f->datalink_hdr), desc.len = frame bytes (f->buffer_len), desc.seed = the IPv6 net_len |
 * proto << 16 as for pico_ipv6_checksum_batch_dev (IPv6 frames; 0 otherwise).
 * Per frame, as pico_ethernet_receive / pico_eth_receive (modules/pico_ethernet.c:180-235):
 *   RX destination filter when mac != NULL (host pointer to the device's 6-byte address,
 *   f->dev->eth->mac): own address, 01:00:5e / 33:33 multicast or broadcast, else V_DROP_L2;
 *   ethertype 0x0806 -> V_ARP (no checksum); 0x0800 -> the IPv4 batch semantics on
 *   (off + 14, len - 14) if the version nibble is 4; 0x86DD -> the IPv6 batch semantics if
 *   it is 6, verdict | V_IPV6; anything else V_DROP_L2.  Frames shorter than 15 bytes are
 *   MALFORMED.  d_out_net is 0 for every non-IPv4 frame.  TX (F_TX, no MAC filter) computes
 *   and, with F_WRITE, stores the IPv4 / IPv6 checksums of the frames the stack built.
 *   F_NXTHDR_DISPATCH (RX) applies to the IPv6 frames as in pico_ipv6_checksum_batch_dev. */
int pico_eth_checksum_batch_dev(void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc, uint32_t n,
                                uint32_t flags, const uint8_t *mac, uint16_t *d_out_net, uint16_t *d_out_transport,
                                uint8_t *d_verdict, void *stream);

/* Forwarding step: pico_ipv4_pre_forward_checks (modules/pico_ipv4.c:1535-1574), which
 * pico_ipv4_forward (:1580-1603) runs on a datagram once route_find has a route for it, for a batch
 * of IPv4 datagrams routed through this host (desc.off -> IPv4 header, desc.len = bytes available,
 * >= 20), IN BATCH ORDER:
 *   hdr->ttl is decremented in place; a datagram whose TTL reaches 0 is V_EXPIRED (the reference
 *   drops it -- and sends pico_notify_ttl_expired, the caller's job -- crc untouched);
 *   every other one gets the reference's `hdr->crc++` (:1556, a native little-endian increment of
 *   the stored field), then:
 *   V_LOCAL_SRC  its source is one of local_addrs[0 .. n_local) (the host's link addresses, as
 *                stored: pico_ipv4_link_get's table, :1559; host memory, n_local <= 32);
 *   V_DUPLICATE  (src, id, dst, proto) equals the last datagram that got this far (:1562-1571);
 *   V_ACCEPT     forwarded: it becomes the last datagram (the caller goes on with NAT, the MTU
 *                check and pico_datalink_send, :1600-1610).
 * d_state (device memory, struct pico_csum_fwd_state) is the reference's static last tuple, carried
 * from one batch to the next; zero it once at start (the reference's initial value: a first datagram
 * with an all-zero tuple is a duplicate).  NULL: a zero state, not kept.  Calls that share a d_state
 * must be ordered (one stream).  Regions past base_len or shorter than 20 bytes are V_MALFORMED,
 * untouched, and leave the state alone.  d_verdict is required (the batch order is resolved through
 * it).  The descriptors of one batch must not overlap: each header is updated by one lane with a
 * plain read-modify-write, so two descriptors on the same header would race on its TTL / crc
 * (the reference, handed the same frame twice, would apply both decrements in sequence).  Three
 * kernel launches on `stream`. */
struct pico_csum_fwd_state {
    uint32_t src;       /* last_src, as stored */
    uint32_t dst;       /* last_dst */
    uint16_t id;        /* last_id, as stored (bytes 4-5 of the header) */
    uint16_t proto;     /* last_proto */
    uint32_t reserved;
};
int pico_ipv4_forward_batch_dev(void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc, uint32_t n,
                                const uint32_t *local_addrs, uint32_t n_local, struct pico_csum_fwd_state *d_state,
                                uint8_t *d_verdict, void *stream);

/* NAT rewrite of a batch of IPv4 datagrams: the frame work of
 * pico_ipv4_nat_outbound / pico_ipv4_nat_inbound (modules/pico_nat.c:424-545) once the host's
 * tuple table has chosen the new address and port.  desc.off -> IPv4 header, desc.len = bytes
 * available; nat[i] for datagram i (8-byte aligned device array):
 *   dir PICO_CSUM_NAT_OUTBOUND: hdr->src = addr, transport sport = port (:509-510, :525-526)
 *   dir PICO_CSUM_NAT_INBOUND:  hdr->dst = addr, transport dport = port (:446-447, :462-463)
 *   dir PICO_CSUM_NAT_NONE:     left as it is (V_UNTOUCHED; the lookup failed)
 * addr and port as they are stored in the frame (network byte order).  TCP and UDP then get
 * their transport checksum recomputed over the whole transport with the pseudo header of the
 * rewritten header -- UDP too, even if its crc was 0 (:461-465) -- and every translated or ICMPv4
 * datagram its header checksum (:478-481, :543-546); ICMPv4 is not rewritten (:466-468); other
 * protocols are V_UNTOUCHED.  All of it is written in place (V_ACCEPT).  As the reference
 * recomputes rather than adjusts, a wrong stored transport checksum comes out right.
 * A fragment (MF or an offset) is V_FRAG and untouched (it reaches reassembly, not NAT:
 * pico_ipv4.c:446-455); infeasible lengths, or a TCP / UDP transport shorter than its header
 * with a record, are V_MALFORMED and untouched.  d_out_net / d_out_transport: the stored
 * values (0 where none); any output pointer may be NULL.  One pass over each datagram: the
 * rewritten words enter the sums as deltas of the old ones (RFC 1624, on full sums). */
#define PICO_CSUM_NAT_NONE     0u
#define PICO_CSUM_NAT_OUTBOUND 1u
#define PICO_CSUM_NAT_INBOUND  2u
struct pico_csum_nat {
    uint32_t addr;      /* new source (outbound) / destination (inbound) address, as stored */
    uint16_t port;      /* new source / destination port, as stored */
    uint8_t dir;        /* PICO_CSUM_NAT_* */
    uint8_t reserved;
};
int pico_ipv4_nat_batch_dev(void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc, uint32_t n,
                            const struct pico_csum_nat *d_nat, uint16_t *d_out_net, uint16_t *d_out_transport,
                            uint8_t *d_verdict, void *stream);

/* IPv4 fragment reassembly fused with the transport check of the reassembled datagram
 * (pico_ipv4_process_frag / pico_fragments_check_complete /
 * pico_fragments_reassemble, modules/pico_fragments.c:129-139,216-239,304-358,499-568, then
 * pico_transport_crc_check, stack/pico_socket.c:1916-1968).  One pass reads each fragment's
 * payload once, writes it into the reassembled datagram and sums it; the reference copies
 * it (memcpy, :334-345) and sums the copy again.
 *   d_frag[]   fragments as pico_ipv4_process_in hands them on (desc.off -> the fragment's
 *              IPv4 header, desc.len = bytes available; header already checked)
 *   d_groups[] 2 uint32 per datagram: first fragment, count -- the fragments one reassembly
 *              tree collects (src / dst / id matched by pico_flow_group_batch_dev, or by the stack), in
 *              arrival order
 *   d_out_desc[] per datagram: output region in d_out (off a multiple of 4, len = capacity;
 *              off = 12 mod 16 puts the transport on a 16-byte line: whole-line stores)
 * Tree order by fragment offset ((frag & 0x1FFF) << 3; a repeated offset keeps the earlier
 * arrival, as pico_tree_insert rejects the later); complete when the offsets are contiguous
 * from 0 up to the first fragment without MF.  The output is the first fragment's 20 header
 * bytes (options are not copied, :332-333) followed by every payload.
 *   d_out_len[g]       transport length of the reassembled datagram, 0 when not reassembled
 *   d_out_transport[g] TCP (always) / UDP (crc != 0) checksum with the pseudo header of the
 *                      copied header (0 = valid; 0 when none is computed)
 *   d_verdict[g]       ACCEPT, L4_BAD, or MALFORMED = not reassembled: incomplete, a fragment
 *                      behind the completing one (the reference's copy loop would write past
 *                      its buffer: reference UB), 20 + len > 65535 (its uint16 allocation size
 *                      wraps), a fragment header or payload past desc.len or base_len, an empty
 *                      group or one of more than 512 fragments, an output region too small.
 * The bytes of an output region are unspecified when its datagram is not reassembled (the
 * gather starts before completeness is known) and past the reassembled datagram's end (a
 * repeated offset's later arrival may have been gathered there); no byte outside the region is
 * written.  Any of the three output pointers may be NULL.  Batches of 512 datagrams or more run
 * on a flat grid whose per-datagram tallies live in library scratch (8 bytes a datagram, kept
 * zero between calls): per calling thread and stream, kept across calls and freed when the
 * thread exits or calls pico_csum_release_thread_scratch; in a call captured into a graph,
 * owned by that graph (freed after the graph is destroyed, by the next eager call or release)
 * -- two executable instances of one captured graph must not run concurrently
 * (pico_csum_set_reasm_flat selects the grid). */
int pico_ipv4_reassemble_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_frag,
                                   uint32_t n_frag, const uint32_t *d_groups, uint32_t n_dgram, void *d_out,
                                   uint64_t out_len, const struct pico_csum_desc *d_out_desc, uint32_t *d_out_len,
                                   uint16_t *d_out_transport, uint8_t *d_verdict, void *stream);

/* IPv6 fragment reassembly fused with the transport check of the reassembled datagram
 * (pico_ipv6_process_frag / pico_fragments_check_complete /
 * pico_fragments_reassemble, modules/pico_fragments.c:73-83,216-239,304-358,432-498).  Arguments
 * as pico_ipv4_reassemble_batch_dev, with d_frag[] -> each fragment's IPv6 header (desc.len =
 * bytes available; desc.seed reserved, 0): the kernel walks each fragment's extension headers as
 * pico_ipv6_extension_headers does (pico_ipv6.c:659-809) -- the transport must lie behind a
 * fragment header -- for net_len, the fragment field (offset = frag & 0xFFF8, more = frag & 1,
 * pico_fragments.c:35-36) and the transport protocol; transport_len = payload_len - (net_len - 40)
 * (pico_ipv6.c:790).  The output is the first fragment's 40-byte fixed header (its extension
 * headers are not copied, :334-338) followed by every payload (out_desc.off = 8 mod 16 puts the
 * transport on a 16-byte line).  The check of the reassembled datagram follows the module the
 * completing fragment hands it to (its transport protocol): TCP / UDP through
 * pico_transport_crc_check with the reference's byte-9 dispatch on the copied header
 * (PICO_CSUM_F_NXTHDR_DISPATCH: by the module instead), ICMPv6 through pico_icmp6_checksum (a
 * verdict for the ND / MLD types only).  Verdicts and the unspecified-bytes rule as for IPv4
 * (40 + len > 65535 and a fragment that does not walk to a fragment header are MALFORMED). */
int pico_ipv6_reassemble_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_frag,
                                   uint32_t n_frag, const uint32_t *d_groups, uint32_t n_dgram, void *d_out,
                                   uint64_t out_len, const struct pico_csum_desc *d_out_desc, uint32_t *d_out_len,
                                   uint16_t *d_out_transport, uint8_t *d_verdict, uint32_t flags, void *stream);

/* IPv4 TX fragmentation: the inverse of pico_ipv4_reassemble_batch_dev, fused with every
 * fragment's header checksum and the transport checksum of the whole datagram (the batch form of
 * pico_socket_xmit_fragments, stack/pico_socket.c:1131-1251, with pico_ipv4_frame_push's len / id /
 * frag / pico_ipv4_checksum per frame, modules/pico_ipv4.c:1039-1079; pico_ipv4_rebound_large,
 * :1464-1510, splits a large ICMP reply by the same rule).  One pass reads each transport byte
 * once, writes it into its fragment and sums it; the reference copies it (memcpy) and sends
 * fragmented UDP with crc = 0 because nothing sums the whole payload (modules/pico_udp.c:119-123).
 *   d_dgram[]  one unfragmented datagram each: desc.off -> a 20-byte IPv4 header (IHL 5), desc.len =
 *              20 + transport bytes (<= 65535), desc.seed = 0 -- what the reassembly batch writes.
 *              vhl, tos, id, ttl, proto, src and dst are taken from the header; its len, frag and
 *              crc fields are not read (the socket and IP layers set them, :1040, :1069, :1079).
 *   split      per = (mtu - 20) & ~7 payload bytes a fragment (mtu >= 28, else -EINVAL): the
 *              reference's rule wherever it places data correctly (mtu - 20 a multiple of 8, e.g.
 *              1500; its frag = (written + 8) >> 3 misplaces data for any other MTU, e.g. the 1280
 *              it uses before a socket has a device -- the evident intent there).  A datagram of
 *              desc.len <= mtu goes out whole, count 1, frag = 0x4000 (DF, :1059); else count =
 *              ceil((len - 20) / per), fragment k carries transport bytes [k per, min((k + 1) per,
 *              len - 20)) behind the input's 20 header bytes with len = 20 + payload, frag =
 *              (k per) >> 3 | 0x2000 on every fragment but the last (DF never), crc =
 *              pico_ipv4_checksum.
 *   d_out_desc[] per datagram: output region in d_out (off any alignment, len = capacity).  Fragment
 *              k starts at off + k frag_stride; frag_stride a multiple of 4, >= 20 + per (else
 *              -EINVAL).  off = 12 mod 16 with a stride that is a multiple of 16 puts every payload
 *              on a 16-byte line (whole-line stores; the reassembly's rule).
 *   d_groups[] 2 uint32 per datagram, the reassembly's layout, read-only: first slot in d_out_frag,
 *              slots reserved.  d_out_frag[first + k] = {fragment k's offset in d_out, 20 + payload,
 *              0}; reserved slots past count = {0, 0, 0}.  A group that reserves exactly count slots
 *              lets d_out, d_out_frag and d_groups go to pico_ipv4_reassemble_batch_dev as they are.
 *   d_out_count[g]     fragments emitted (0 when MALFORMED)
 *   d_out_transport[g] the whole datagram's transport checksum, its crc field read as zero when it
 *              lies inside the transport, by the TX rule of the fused batches: TCP and UDP with the
 *              pseudo header of the template, ICMPv4 without one, 0 for other protocols; UDP is
 *              computed and stored as it is, as the NAT batch does (pico_nat.c:464-465).  With
 *              PICO_CSUM_F_WRITE it is stored into that crc field (in the fragment that holds it:
 *              the first unless per < 24); without, the transport is copied verbatim -- the
 *              reference's bytes, UDP's crc = 0 included.  Other flags: -EINVAL.
 *   d_verdict[g]       ACCEPT, or MALFORMED = no byte of the region is written: a datagram past
 *              base_len, len < 20 or > 65535, IHL != 5, fewer reserved slots than count, slots past
 *              n_frag (then no slot is written either), an output region too small for
 *              (count - 1) frag_stride + the last fragment or past out_len.  Its count is 0 and its
 *              slots are {0, 0, 0}.
 * No byte outside [d_out_desc[g].off, + len) is written, and inside it only the fragments' own
 * bytes (gaps between fragments keep their contents).  Reads follow the whole-16-byte-block rule
 * above.  d_out_frag, d_out_count, d_out_transport and d_verdict may each be NULL.  Regions and slot
 * ranges of different datagrams must not overlap.  One workgroup per datagram, one launch. */
int pico_ipv4_fragment_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_dgram,
                                 uint32_t n_dgram, uint32_t mtu, const uint32_t *d_groups, uint32_t n_frag, void *d_out,
                                 uint64_t out_len, const struct pico_csum_desc *d_out_desc, uint32_t frag_stride,
                                 struct pico_csum_desc *d_out_frag, uint32_t *d_out_count, uint16_t *d_out_transport,
                                 uint8_t *d_verdict, uint32_t flags, void *stream);

/* IPv6 TX fragmentation: the inverse of pico_ipv6_reassemble_batch_dev, fused with the transport
 * checksum of the whole datagram -- mandatory for UDP over IPv6.  The reference has no sending side
 * to mirror: pico_socket_xmit_fragments "Can't fragment IPv6" and cuts the datagram to one MTU
 * (stack/pico_socket.c:1179-1185).  The split is RFC 8200 4.5's, and it is pinned to the reference's
 * receiver: pico_ipv6_process_frag (modules/pico_fragments.c:432-498), compiled unmodified,
 * reassembles the fragments written here into the datagram they were cut from
 * (tests/golden/make_ref_fragtx6.py).  Everything not said here is as pico_ipv4_fragment_batch_dev
 * states it.
 *   d_dgram[]  one unfragmented datagram each: desc.off -> the 40-byte IPv6 fixed header followed
 *              directly by the transport (no extension headers: an unfragmentable part is out of
 *              scope), desc.len = 40 + T transport bytes, 40 <= len <= 65535 (what the IPv6 reassembly
 *              batch accepts back), desc.seed = the 32-bit fragment identification in host order (the
 *              host keeps the counter, as it keeps id for the segmentation batch).  The version nibble
 *              (6), class and flow label, nxthdr, hop limit, src and dst are taken from the header;
 *              its payload-length field is not read.  nxthdr names the transport: an extension
 *              header's value (0, 43, 44, 50, 51, 60, 135) is MALFORMED.
 *   split      per = (mtu - 48) & ~7 payload bytes a fragment (mtu >= 56, else -EINVAL; IPv6's minimum
 *              of 1280 is the host's policy).  A datagram of desc.len <= mtu goes out whole, count 1:
 *              its 40 header bytes with payload length = T and nxthdr unchanged, then the transport;
 *              no fragment header; slot length = desc.len.  Else count = ceil(T / per), fragment k
 *              carries transport bytes [k per, min((k + 1) per, T)) behind 48 header bytes: bytes 0-3
 *              and 7-39 the template's, 4-5 = be16(8 + payload), 6 = 44, then the fragment header:
 *              40 = the template's nxthdr, 41 = 0, 42-43 = be16(k per | 1 on every fragment but the
 *              last), 44-47 = be32(seed).  d_out_frag[first + k] = {off + k frag_stride, 48 + payload, 0}.
 *   d_out_desc[] as for IPv4; frag_stride a multiple of 4, >= 48 + per (else -EINVAL).  off = 0 mod
 *              16 with a stride that is a multiple of 16 puts every payload on a 16-byte line.
 *   d_groups[] as for IPv4.  A group that reserves exactly count slots lets d_out, d_out_frag and
 *              d_groups go to pico_ipv6_reassemble_batch_dev as they are.  Its output header is then
 *              fragment 0's (that batch's rule): nxthdr 44, payload length 8 + per -- a reassembled
 *              datagram needs its byte 6 set by the host before it can be fragmented again.
 *   d_out_transport[g] the value pico_ipv6_checksum_batch_dev reports with PICO_CSUM_F_TX for the same
 *              datagram unfragmented: TCP (crc field at byte 16) / UDP (6) / ICMPv6 (2) over the
 *              transport with the field read as zero and struct pico_ipv6_pseudo_hdr from the
 *              template's addresses, T and nxthdr, stored as computed; 0 for any other protocol and
 *              for a transport shorter than its header (20 / 8 / 4 bytes: that batch's MALFORMED,
 *              here fragmented all the same).  With PICO_CSUM_F_WRITE a computed value is stored
 *              into the fragment that holds the field: kf = crc_at / per, at byte 48 + crc_at -
 *              kf per (a whole datagram: 40 + crc_at); without, the transport is copied verbatim.
 *              Other flags: -EINVAL.
 *   d_verdict[g]       ACCEPT, or MALFORMED = no byte of the region is written, count 0, slots
 *              {0, 0, 0}: a datagram past base_len, len < 40 or > 65535, version not 6, an
 *              extension-header nxthdr, fewer reserved slots than count, slots past n_frag (then no
 *              slot is written either), a region too small for (count - 1) frag_stride + the last
 *              fragment or past out_len.  Every check is made before the first store.
 * Writes, reads, NULL outputs and overlap rules as for IPv4.  One workgroup per datagram, one launch. */
int pico_ipv6_fragment_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_dgram,
                                 uint32_t n_dgram, uint32_t mtu, const uint32_t *d_groups, uint32_t n_frag, void *d_out,
                                 uint64_t out_len, const struct pico_csum_desc *d_out_desc, uint32_t frag_stride,
                                 struct pico_csum_desc *d_out_frag, uint32_t *d_out_count, uint16_t *d_out_transport,
                                 uint8_t *d_verdict, uint32_t flags, void *stream);

/* TCP send segmentation (what a NIC calls TSO): one header template and one long payload per
 * connection become the segment-sized frames of a pico_socket_write, each with its own IPv4 header
 * checksum and TCP checksum, in one pass that reads each payload byte once.  The batch form of
 * pico_socket_xmit / pico_socket_xmit_one (stack/pico_socket.c:1322-1358, :1070-1127: a frame per
 * `space` bytes, memcpy of the payload), pico_tcp_push (modules/pico_tcp.c:3127-3157: seq =
 * snd_last + 1, snd_last += payload_len), pico_tcp_output / tcp_add_options_frame (:2924-2998,
 * :633-660), tcp_send (:968-985: crc = short_be(pico_tcp_checksum(f))) and pico_ipv4_frame_push
 * (modules/pico_ipv4.c:1039-1079: len, id = ipv4_progressive_id++, frag = DF, pico_ipv4_checksum);
 * the reference touches every payload byte twice (memcpy, checksum) and every header twice.  The
 * rule below reproduces, byte for byte, the data segments the compiled reference emits for a write
 * within one millisecond of its clock, or on a connection without the timestamp option
 * (tests/golden/make_ref_tcpseg.py, tests/test_ref_tcpseg.py).  The TX batches above checksum frames the host has built one
 * by one; this one builds them.
 *   d_stream[g] one send unit: desc.off -> a network header, the TCP header and the payload, contiguous;
 *              desc.len = the byte count of all of it (the payload may be far longer than 65535);
 *              desc.seed = `per`, the payload bytes a segment (the reference's `space`,
 *              pico_socket_xmit_avail_space: the socket's MSS minus the option overhead -- per
 *              connection, so per stream).  The version nibble selects the family: IPv4 with IHL 5
 *              and proto 6 (N = 20), or IPv6 with nxthdr 6 and no extension header (N = 40).  thl =
 *              4 (TCP byte 12 >> 4), 20..60; H = N + thl; P = desc.len - H.
 *   split      count = max(1, ceil(P / per)) (P = 0: one bare-header frame).  Segment k carries
 *              payload bytes [k per, min((k + 1) per, P)) behind a copy of the H template bytes with
 *              IPv4: len = H + payload, id = template id + k (mod 2^16), frag = 40 00 (DF,
 *              pico_ipv4.c:1059), crc = pico_ipv4_checksum; IPv6: payload length (bytes 4-5) = thl +
 *              payload; TCP: seq = template seq + k per (mod 2^32), crc = pico_tcp_checksum with the
 *              pseudo header of the template's addresses, proto 6 and length thl + payload (struct
 *              pico_ipv4_pseudo_hdr / pico_ipv6_pseudo_hdr).  Everything else -- ports, ack, flags,
 *              window, urgent pointer, options, tos, ttl / hop limit, addresses, flow label -- is the
 *              template's on every segment.  The reference puts PSH|ACK on every segment too (PSH is
 *              not moved to the last); it stamps each segment's timestamp option with the clock's
 *              millisecond as it sends it (tcp_add_options_frame: tsval = TCP_TIME), the batch copies
 *              the template's: per-segment options are out of scope, and a later tsval means a new
 *              send unit.  The template's IPv4 len, frag and crc, its IPv6 payload length and its TCP
 *              crc are not read.
 *   d_out_desc[] per stream: output region in d_out (off any alignment, len = capacity).  Segment k
 *              starts at off + k seg_stride; seg_stride a multiple of 4, >= 40 (else -EINVAL).  off + H
 *              = 0 mod 16 with a stride that is a multiple of 16 puts every payload on a 16-byte
 *              line (whole-line stores; off = 12 mod 16 for IPv4 with thl 32).
 *   d_groups[] 2 uint32 per stream, the fragmentation batch's layout, read-only: first slot in
 *              d_out_seg, slots reserved.  d_out_seg[first + k] = {segment k's offset in d_out, H +
 *              payload, 0}; reserved slots past count = {0, 0, 0}.  d_out and d_out_seg go to
 *              pico_ipv4_checksum_batch_dev / pico_ipv6_checksum_batch_dev as they are (RX mode:
 *              every frame ACCEPT, both results 0; IPv6 with PICO_CSUM_F_NXTHDR_DISPATCH, the default
 *              dispatch reads the source address's second byte).
 *   d_out_count[g]     segments emitted (0 when MALFORMED)
 *   d_verdict[g]       ACCEPT, or MALFORMED = no byte of the region is written, count 0, slots {0, 0,
 *              0}; checked in an order that never reads past desc.len: a stream past base_len, len <
 *              1, a version other than 4 / 6, len < N, IHL != 5, proto / nxthdr != 6, len < N + 20,
 *              thl < 20, len < H, per = 0, a frame length that does not fit its 16-bit field (IPv4: H +
 *              min(per, P) > 65535, IPv6: thl + min(per, P) > 65535), H + min(per, P) > seg_stride,
 *              fewer reserved slots than count, slots past n_seg (then no slot is written either), an
 *              output region too small for (count - 1) seg_stride + the last frame or past out_len.
 * No byte outside [d_out_desc[g].off, + len) is written, and inside it only the frames' own bytes
 * (gaps between frames keep their contents).  Reads follow the whole-16-byte-block rule above.
 * d_out_seg, d_out_count and d_verdict may each be NULL.  Regions and slot ranges of different
 * streams must not overlap.  flags is reserved: anything but 0 is -EINVAL.  The host keeps the TCP
 * state (INTEGRATION.md 5a''): after the call snd_last advances by P and the id counter by count.
 * One launch, one workgroup per stream (four waves; one wave in batches of 3072 streams or more that
 * reserve at most 16 slots a stream on average); results never depend on the launch shape. */
int pico_tcp_segment_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_stream,
                               uint32_t n_stream, const uint32_t *d_groups, uint32_t n_seg, void *d_out,
                               uint64_t out_len, const struct pico_csum_desc *d_out_desc, uint32_t seg_stride,
                               struct pico_csum_desc *d_out_seg, uint32_t *d_out_count, uint8_t *d_verdict,
                               uint32_t flags, void *stream);

/* TCP receive coalescing (what a NIC calls LRO / GRO): each connection's received segments are verified
 * and the in-order byte stream is delivered into one contiguous region, in one pass that reads each
 * delivered payload byte once.  The inverse of pico_tcp_segment_batch_dev -- its d_out / d_out_seg go
 * in as they are -- and the batch form of pico_transport_crc_check (stack/pico_socket.c:1916-1968) +
 * tcp_data_in (modules/pico_tcp.c:1717-1776, with segment_from_frame's copy, :97-119) +
 * pico_tcp_read (:1149-1182, a second copy): three passes over every received byte in the reference.
 *   d_seg[]    one received frame each: desc.off -> the network header, desc.len = bytes available from
 *              there (nothing past it or past base_len is read, with the whole-16-byte-block read rule
 *              above), desc.seed = 0.  The version nibble selects the family: IPv4 (any IHL >= 5, proto
 *              6) or IPv6 with nxthdr 6 and no extension header.
 *   d_groups[] 2 uint32 per connection: first segment, count, IN ARRIVAL ORDER (pico_flow_group_batch_dev
 *              matches the 4-tuple on the device, against the host's connection table; a host that has
 *              matched it itself passes its own groups)
 *   d_conn[]   2 uint32 per connection: rcv_nxt, cflags.  cflags bit 0 = the connection's sack_ok; the
 *              other bits are reserved and must be 0.
 *   d_out_desc[] per connection: output region in d_out (off any alignment -- off = 0 mod 16: whole-line
 *              stores; len = capacity, which acts as the receive window)
 *   flags      reserved: anything but 0 is -EINVAL
 * Per segment, its FIRST outcome in the reference's order (d_seg_verdict[i], written for every segment
 * of every group that lies inside n_seg):
 *   1. MALFORMED  the frame past base_len, a header past desc.len, an infeasible IPv4 length, a version
 *                 other than 4 / 6, proto / nxthdr != 6, IPv6 40 + payload length > desc.len, a transport
 *                 shorter than 20 bytes, thl < 20 or thl > the transport length (tcp_data_in, :1735);
 *      NET_BAD    the IPv4 header checksum;  MALFORMED again: an invalid source, the evil bit, IHL < 5;
 *      FRAG       MF or an offset: route the frame to the reassembly.
 *      These are pico_ipv4_checksum_batch_dev's RX rules, in its order.
 *   2. TCP_CTRL   flags other than ACK or PSH|ACK, or a zero-length payload: for the host's state
 *                 machine.  The segment is not part of the chain: it is treated as if it had not arrived.
 *   3. The chain, among the remaining candidates: cur = rcv_nxt; repeatedly take the EARLIEST ARRIVAL with
 *      seq == cur that has not been struck, cur += payload_len (mod 2^32).  With sack_ok the search is
 *      over the whole group (the reference queues a segment ahead of rcv_nxt, tcp_data_in_high_segment,
 *      :1693-1714, and scrolls over it later, :1677-1683; a second arrival of a queued seq is refused
 *      by pico_tree_insert, :201).  Without, a segment counts only if it arrives AFTER the previously
 *      taken one (the reference drops a high segment, :1696): the search starts behind the last taken
 *      index.  A member whose bytes do not fit in the remaining capacity ends the chain.  A member is
 *      copied to out + (seq - rcv_nxt) and its TCP checksum is verified from the bytes copied: IPv4
 *      with pico_tcp_checksum_ipv4's pseudo header; IPv6 ALWAYS with the TCP pseudo header
 *      (pico_tcp_checksum_ipv6) -- what PICO_CSUM_F_NXTHDR_DISPATCH selects in the RX batch; the
 *      reference's byte-9 dispatch quirk is deliberately not followed here: a coalesced stream must not
 *      depend on an address byte.  Every member that fails is STRUCK (L4_BAD, for good) and the chain is
 *      planned again without the struck ones, until a planned chain verifies in full: a later
 *      retransmission of that seq may take a struck member's place.  That is what the reference does in
 *      arrival order, since a bad segment never reaches the socket.
 *   4. With the chain's end E final: its members ACCEPT; a candidate not on it (and not struck) with seq
 *      before E (pico_seq_compare) TCP_OLD; one at or beyond E TCP_HELD -- not delivered in this call,
 *      its payload not read, so its checksum not judged: the host resubmits held segments with the next
 *      burst if the connection has SACK, and forgets them otherwise.
 *   d_out_len[g]  E - rcv_nxt: the host's new rcv_nxt is rcv_nxt + out_len
 *   d_verdict[g]  ACCEPT (out_len 0 included), or MALFORMED = nothing of the region is written, out_len 0,
 *              every segment of the group MALFORMED (where the group lies inside n_seg): an empty group or
 *              one past n_seg, more than 512 segments, a region past out_len, reserved cflags.
 * Bytes [0, out_len) of the region are the stream; region bytes past out_len are unspecified (a struck
 * member, or a member of a chain planned before a strike, may have been copied there); no byte outside
 * the region is written.  d_out_len, d_seg_verdict and d_verdict may each be NULL.  Regions and groups
 * of different connections must not overlap.
 * One documented difference: pico_tcp_read walks the tree by overlap (:1164-1171), so with a queued
 * segment that partly overlaps the chain it reads past rcv_nxt, out of that segment's tail; the batch
 * delivers up to rcv_nxt, what the stack has ACKed.  For segments cut from one consistent byte stream
 * the first out_len bytes agree.  No queue limit (PICO_DEFAULT_SOCKETQ) is enforced: the capacity is
 * the window.  The host keeps the TCP state: ACKs, tcp_ack, FIN / RST, SACK
 * blocks.  One launch, one workgroup per connection (four waves; one wave in batches of 3072
 * connections or more with at most 16 segments a connection on average), no library scratch; results
 * never depend on the launch shape. */
int pico_tcp_coalesce_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_seg,
                                uint32_t n_seg, const uint32_t *d_groups, const uint32_t *d_conn, uint32_t n_conn,
                                void *d_out, uint64_t out_len, const struct pico_csum_desc *d_out_desc,
                                uint32_t *d_out_len, uint8_t *d_seg_verdict, uint8_t *d_verdict, uint32_t flags,
                                void *stream);

/* The burst's ACKs: one launch behind pico_tcp_coalesce_batch_dev on the same stream, reading the
 * coalescing's own inputs and outputs.  It finishes the checksum verdicts the coalescing left open and
 * writes one ready-to-send ACK frame per connection, SACK blocks and both checksums included.  The batch
 * form of tcp_data_in_send_ack -> tcp_send_ack -> tcp_send_empty (modules/pico_tcp.c:1716-1725, :1324-1327,
 * :1286-1322) with tcp_sack_prepare (:1597-1657), tcp_options_size (:703-731), tcp_add_options /
 * tcp_add_sack_option (:582-617, :560-580), tcp_set_space (:681-700) and pico_ipv4_frame_push
 * (modules/pico_ipv4.c:1039-1079).
 *   d_base, d_seg, d_groups, d_conn   as the coalescing took them
 *   d_out_len, d_seg_verdict          as the coalescing wrote them (both required); d_seg_verdict is updated
 *              in place
 *   d_tmpl[g]  desc.off -> the connection's header template in d_tmpl_base: a network header followed by a
 *              20-byte TCP header, desc.len >= N + 20 (nothing past it or past tmpl_len is read).  The family
 *              rule and its order are pico_tcp_segment_batch_dev's: the version nibble selects IPv4 (IHL 5,
 *              proto 6; N = 20) or IPv6 (nxthdr 6, no extension header; N = 40).  Taken from it: the addresses,
 *              tos / flow label, ttl / hop limit, the IPv4 id, the ports, seq (the host's snd_nxt), the low
 *              nibble of TCP byte 12 (the reference's `jumbo`) and the urgent pointer.  Its own len / frag /
 *              crc / ack / rwnd / flags / thl are not read.
 *   d_ack[g]   struct pico_csum_tcp_ack: space = the free receive space BEFORE this burst (tcpq_in.max_size -
 *              tcpq_in.size), tsval / tsecr in host order, aflags bit 0 = ts_ok (the rest reserved, 0)
 *   d_out_desc[g]  the frame's region in d_out (off any alignment; len >= the frame: 100 bytes always do)
 *   flags      reserved: anything but 0 is -EINVAL
 * Per connection g, with rcv' = rcv_nxt + d_out_len[g]:
 *   1. Every segment of the group whose verdict is TCP_OLD or TCP_HELD is verified with pico_tcp_checksum,
 *      with the coalescing's parse and pseudo-header rules (IPv4: pico_tcp_checksum_ipv4; IPv6: always the
 *      TCP pseudo header) and its read rules; each payload byte is read once and nothing is copied.  One that
 *      fails becomes L4_BAD in d_seg_verdict.  Every other verdict stays as it is (a segment marked TCP_OLD /
 *      TCP_HELD that does not parse as a data segment was not marked by the coalescing: it is left alone and
 *      counts for nothing).
 *   2. An ACK is due when at least one segment of the group is now ACCEPT, TCP_OLD or TCP_HELD: the segments
 *      that reach tcp_data_in, each of which draws a tcp_send_ack in the reference.  Otherwise nothing is
 *      written and d_out_ack[g] = {0, 0, 0} (d_verdict[g] ACCEPT).
 *   3. The SACK blocks, with sack_ok (cflags bit 0) only -- without it the reference drops a high segment
 *      (:1696), so held segments contribute nothing.  The queue is the verified TCP_HELD segments, unique by
 *      seq with the earliest arrival kept (pico_tree_insert refuses the later one), in ascending order of
 *      seq - rcv' (pico_seq_compare's order: a held segment lies at or beyond rcv').  tcp_sack_prepare is
 *      applied to that queue and rcv' LITERALLY, with the reference's own first_segment / next_segment
 *      (:161-179) and its quirks: next_segment is not the tree's successor but the segment that starts
 *      exactly where this one ends, or none, so the walk follows ONE contiguous run from the queue's lowest
 *      segment and ends at its first gap -- in practice at most one block, the lowest held run, and later
 *      runs are never reported; at most 3 blocks, pushed to the front of the list (emitted highest-first);
 *      the segment that breaks a run closes the open block and is itself skipped; left == 0 means "no open
 *      block" (a run starting at seq 0 loses its first segment); and `pkt->seq < rcv_nxt` is a raw compare
 *      (past a 2^32 wrap a held segment's seq is below rcv': skipped).
 *   4. The window (tcp_set_space): space_after = max(0, space - d_out_len[g] - held), held = the payload bytes
 *      of the queue (with sack_ok only: the bytes the reference's tcpq_in holds); while space_after > 0xFFFF it
 *      is halved and shift incremented; rwnd = (uint16)space_after, the WS option carries shift.
 *   5. The options (flags = ACK): WS (03 03 shift), then timestamps (08 0a tsval tsecr, with ts_ok), then the
 *      SACK option (05, 2 + 8 b, the blocks) when there are blocks; the area's size is those bytes + 1
 *      (tcp_options_size counts an END) rounded up to a multiple of 4, the rest NOOP (01) with END (00) as
 *      the last byte.  thl = 20 + that size: 24 ... 60.
 *   6. The frame, N + thl bytes at d_out + d_out_desc[g].off: the template with flags = 0x10, ack = rcv',
 *      rwnd, thl and the options; IPv4 len, frag = 40 00 and crc = pico_ipv4_checksum; the IPv6 payload
 *      length; the TCP crc with the pseudo header of the template's addresses.  d_out_ack[g] = {that offset,
 *      N + thl, 0}: with d_out, the input of the TX path or of pico_ipv4_checksum_batch_dev /
 *      pico_ipv6_checksum_batch_dev as it is.
 *   d_verdict[g]  ACCEPT, or MALFORMED = nothing of the region is written, d_out_ack[g] = {0, 0, 0} and the
 *              group's segment verdicts are left as they came: an empty group, one past n_seg or of more than
 *              512 segments; reserved cflags or aflags; a template past tmpl_len or one that fails the family
 *              checks; an output region past out_len or smaller than the frame.
 * No byte outside a region is written, and inside it only the frame's own bytes.  d_out_ack and d_verdict
 * may each be NULL.  Documented differences from the reference: ONE ACK per connection per burst (the
 * reference sends one per data segment: INTEGRATION.md 5a-rx); blocks whenever verified held segments exist
 * (tcp_sack_prepare runs only on a high segment, skips while earlier blocks are pending, and starts at
 * delivered segments the application has not read yet: the batch's queue holds the held segments only,
 * the delivered bytes being in the reader's region); tsecr is the
 * host's (the reference echoes the last parsed segment's tsval); tcp_sack_prepare's quirks are kept, not
 * repaired.  The host keeps tsecr, the delayed-ACK policy and tcp_ack.
 * Host checks, -EINVAL before any launch: a NULL required pointer; d_seg, d_tmpl, d_out_desc or d_out_ack not
 * 16-byte aligned; d_groups, d_conn, d_out_len or d_ack not 4-byte aligned; flags != 0.  n_conn == 0 is a
 * no-op; without a device -ENODEV.  One launch (the coalescing's two shapes, chosen the same way), no
 * allocation, no library scratch, no host synchronisation: capturable behind the coalescing as a straight
 * line.  Results never depend on the launch shape. */
struct pico_csum_tcp_ack {       /* 16 bytes, per connection, host-filled */
    uint32_t space;              /* free receive space before this burst */
    uint32_t tsval, tsecr;       /* host order; written big-endian when ts_ok */
    uint32_t aflags;             /* bit 0 = ts_ok; the rest reserved, must be 0 */
};
int pico_tcp_ack_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_seg, uint32_t n_seg,
                           const uint32_t *d_groups, const uint32_t *d_conn, uint32_t n_conn, const uint32_t *d_out_len,
                           uint8_t *d_seg_verdict, const void *d_tmpl_base, uint64_t tmpl_len,
                           const struct pico_csum_desc *d_tmpl, const struct pico_csum_tcp_ack *d_ack, void *d_out,
                           uint64_t out_len, const struct pico_csum_desc *d_out_desc, struct pico_csum_desc *d_out_ack,
                           uint8_t *d_verdict, uint32_t flags, void *stream);

/* A burst's ICMPv4 answers: the echo replies and the notices (destination unreachable, time exceeded,
 * parameter problem) that the verdicts of the RX, forwarding and reassembly batches call for, each built
 * on the device as a finished IPv4 datagram in its own output region.  The batch form of
 * pico_icmp4_process_in (modules/pico_icmp4.c:47-85) with pico_icmp4_checksum (:30-41), pico_ipv4_rebound
 * and pico_ipv4_frame_push (modules/pico_ipv4.c:1512-1533, :1039-1079), and of pico_icmp4_notify
 * (modules/pico_icmp4.c:106-141; its callers: stack/pico_stack.c:82-183, pico_ipv4.c:1553, :1595-1597).  An
 * echo reply is a copy and a sum of up to 64 KiB: one pass reads each transport byte once, where the
 * reference rewrites the frame, sums the whole transport again and pushes it.  The host chooses which
 * datagram gets which record, looks up the route (src), keeps the id counter, limits the rate and keeps
 * ping_recv_reply.
 *   d_desc[i]  the datagram that is answered: desc.off -> its IPv4 header, desc.len = bytes available from
 *              there (nothing past it or past base_len contributes; reads follow the whole-16-byte-block
 *              rule above); desc.seed is not read.
 *   d_req[i]   struct pico_csum_icmp4_req, host-filled: src = the answer's source (the address of the link
 *              the route to the asker uses, :1055, as stored in a frame), id = the IPv4 id (host order,
 *              :1041), type 0 = answer as pico_icmp4_process_in does, type 3 / 11 / 12 with any code =
 *              the notice to send.
 *   d_out_desc[i]  the answer's region in d_out (off any alignment, len = capacity).
 *   d_out_ans[i]   {the answer's offset in d_out, its length, 0} -- with d_out, the input of the TX path,
 *              of pico_ipv4_checksum_batch_dev or of pico_ipv4_fragment_batch_dev as it is -- or {0, 0, 0}.
 * Echo (type 0).  A record is an echo request when it parses -- version 4, IHL >= 5, proto 1, IHL 4 + 8 <=
 * len field <= desc.len -- and its ICMP type is 8 (:55).  One that parses with another ICMP type is
 * V_UNTOUCHED (the NAT batch's bit) and nothing is written: echo replies, unreachables and the rest stay
 * the host's (ping_recv_reply :77, pico_ipv4_unreachable :74).
 *   duplicates (:61-69)  an echo request whose (id, seq) equals that of the nearest earlier echo request of
 *              the batch -- answered or not: a dropped duplicate leaves the statics equal -- or, when there
 *              is none, of the carried state with seen != 0, is V_DUPLICATE and nothing is written.  The
 *              compare ignores the source address, as the reference's does.  After the batch d_state holds
 *              the last echo request's pair, as stored in its frame, and seen = 1 (firstpkt, last_id,
 *              last_seq); a batch without an echo request leaves it as it was.  d_state NULL: nothing is
 *              carried in and nothing is kept.  A MALFORMED record takes no part.
 *   the answer  20 + T bytes, T = len field - IHL 4: the header 45, tos 0, len, req.id, the request's frag
 *              field as it lies (f->frag = short_be(hdr->frag), pico_ipv4.c:402, comes back through
 *              :1072-1075), ttl 64, proto 1, pico_ipv4_checksum (:1079), src = req.src, dst = the request's
 *              source (:1527); then the request's T transport bytes with type 0 (:56) and crc =
 *              pico_icmp4_checksum over the bytes AS COPIED -- never derived from the request's crc: the
 *              reference does not verify an echo request's checksum and answers a corrupted one with a
 *              valid reply.  Bytes behind the datagram (padding, a trailer) are not copied.  tos 0 / ttl
 *              64 are what send_tos / send_ttl of a received frame give (:1050-1057), as the captured
 *              replies show (tests/golden/ref_icmp4_cases.npz).
 * Notices (type 3, 11, 12; any code): pico_icmp4_notify literally.  q = min(len field, 28) bytes are quoted
 * from the IPv4 header on WHATEVER the IHL (:118-126, :137: with options the quote holds option bytes where
 * the transport's first 8 would be -- kept), as they lie (behind the forwarding batch: with the decremented
 * ttl).  The answer is 20 + 8 + q bytes: the header as above with frag 0 (the answer frame's own f->frag),
 * then type, code, crc, 00 00, 05 dc (ipm_void, ipm_nmtu = 1500 on every notice, :133-134), the quote; dst =
 * the datagram's source (:139).  Nothing but the len field is parsed.
 *   d_verdict[i]  ACCEPT = the answer is written and d_out_ans[i] set; V_UNTOUCHED, V_DUPLICATE (the
 *              forwarding batch's bit) as above; MALFORMED = nothing of the region is written: a descriptor
 *              past base_len or of fewer than 20 bytes, a req.type outside {0, 3, 11, 12}, an echo record
 *              that fails the parse, a notice with len field < 20 or q > desc.len, and -- for a record that
 *              would be answered -- a region past out_len or smaller than the answer.  For all three
 *              d_out_ans[i] = {0, 0, 0}.
 * No byte outside a region is written, and inside it only the answer's own bytes.  Regions must not
 * overlap.  Ids of unanswered records are simply not used (the reference's single counter would not skip
 * them; the peer cannot tell).  Documented differences from the reference: (1) a request with IPv4 options
 * is answered with a 20-byte header followed by its transport -- the reference pushes vhl = 45 (:1039) over
 * a header that still holds the options, which no receiver reads as a reply; the evident intent is restated,
 * as the fragmentation batch does for frag; (2) an answer longer than the MTU is written whole (len up to
 * 65535) where the reference splits it (pico_ipv4_rebound_large, :1464-1510): it goes through
 * pico_ipv4_fragment_batch_dev unchanged, which states the same split.
 * Host checks, -EINVAL before any launch: a NULL required pointer (all but d_state and d_out_ans); d_desc,
 * d_out_desc or d_out_ans not 16-byte aligned; d_req or d_state not 4-byte aligned; flags != 0 (reserved).
 * n == 0 is a no-op; without a device -ENODEV.  Four launches on one stream (verdicts; the duplicates'
 * backward scan; one wave per two records for the answers, per record when base_len >= 1024 n; one
 * workgroup for the state -- three without d_state), no allocation, no library scratch, no spin-wait, no
 * host synchronisation: capturable behind the batch whose verdicts chose the records.  Results never depend
 * on the launch shape. */
struct pico_csum_icmp4_req {   /* 8 bytes, per record, host-filled */
    uint32_t src;              /* the answer's source: the link address the route to the asker uses, as stored in a frame */
    uint16_t id;               /* the IPv4 id to use, host order */
    uint8_t  type, code;       /* type 0: answer as pico_icmp4_process_in does (echo); 3 / 11 / 12: the notice to send */
};
struct pico_csum_icmp4_state { uint32_t seen; uint16_t id, seq; };   /* process_in's statics: firstpkt, last_id, last_seq */
int pico_icmp4_reply_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc, uint32_t n,
                               const struct pico_csum_icmp4_req *d_req, struct pico_csum_icmp4_state *d_state,
                               void *d_out, uint64_t out_len, const struct pico_csum_desc *d_out_desc,
                               struct pico_csum_desc *d_out_ans, uint8_t *d_verdict, uint32_t flags, void *stream);

/* A burst's ICMPv6 answers, the IPv6 twin of the batch above: the echo replies and the notices (destination
 * unreachable, packet too big, time exceeded, parameter problem), each built on the device as a finished
 * IPv6 datagram in its own output region.  The batch form of pico_icmp6_process_in /
 * pico_icmp6_send_echoreply (modules/pico_icmp6.c:94-133, :61-92) with pico_icmp6_checksum (:38-55) and
 * pico_ipv6_frame_push (modules/pico_ipv6.c:1324-1339, the header :1283-1322), and of pico_icmp6_notify
 * (modules/pico_icmp6.c:153-227) behind its wrappers (:229-293).  The IPv6 answers are the heavier ones: the
 * checksum covers a 40-byte pseudo header, and a notice quotes up to 1232 bytes of the datagram, copied and
 * summed, where an ICMPv4 notice quotes 28.  There is NO state argument: the reference keeps none for
 * ICMPv6 -- pico_icmp6_process_in has no duplicate statics, and the compiled stack answers the same
 * (id, seq) every time it arrives (tests/golden/ref_icmp6_cases.npz).  The host chooses which datagram gets
 * which record, looks up the route (src), limits the rate and keeps the ping client.
 *   d_desc[i]  the datagram that is answered: desc.off -> its IPv6 header, desc.len = bytes available from
 *              there (nothing past it or past base_len contributes; reads follow the whole-16-byte-block
 *              rule above); desc.seed is not read.
 *   d_req[i]   struct pico_csum_icmp6_req, host-filled: src = the answer's source where the rules below call
 *              for it (the address of the link the route to the asker uses), hop = the answer's hop limit
 *              (the device's hostvars.hoplimit), type 0 = answer as pico_icmp6_process_in does, type 1 / 2 /
 *              3 / 4 with any code = the notice to send, arg = type 4's pointer or type 2's MTU (host order).
 *   d_out_desc[i]  the answer's region in d_out (off any alignment, len = capacity).
 *   d_out_ans[i]   {the answer's offset in d_out, its length, 0} -- with d_out, the input of the TX path or of
 *              pico_ipv6_checksum_batch_dev as it is -- or {0, 0, 0}.
 * Echo (type 0).  A record parses when its version is 6, 40 + payload-length field <= desc.len and the
 * extension-header walk stays inside the payload -- the IPv6 RX batch's walk (hop-by-hop 0, routing 43,
 * destination options 60; pico_ipv6_extension_headers, modules/pico_ipv6.c:707-809, with the sequence check
 * before it).  It is an echo request when the walk ends at next header 58 with at least 8 transport bytes
 * and ICMPv6 type 128.  A walk that ends at 58 with another type, at a fragment header, at any other
 * protocol or at a header the reference discards is V_UNTOUCHED and nothing is written: neighbour
 * discovery, MLD, echo replies and unreachables stay the host's (:104-131).  An infeasible length (a walk
 * that would leave the payload, fewer than 8 transport bytes) is V_MALFORMED.
 *   the answer  40 + T bytes, T = payload-length field - the extension headers' bytes: 60 00 00 00, len T,
 *              nxthdr 58, req.hop, src = the request's destination -- unless its first byte is 0xff: then
 *              req.src (ipv6_push_hdr_adjust, :1283-1289: a multicast source is replaced by the link's
 *              address) --, dst = the request's source; then 81 00, crc, the request's transport bytes
 *              4 .. T.  crc = pico_icmp6_checksum over the pseudo header (src, dst, T, 58) and the bytes AS
 *              COPIED -- never derived from the request's crc: the reference answers a corrupted request
 *              with a valid reply.  The answer never carries the request's extension headers (the reply is
 *              a freshly allocated frame, :68).
 * Notices (type 1, 3, 4; any code): pico_icmp6_notify literally.  Only the payload-length field is parsed.
 * q = min(40 + payload-length field, 1232) bytes are quoted from the IPv6 header on as they lie.  The answer
 * is 48 + q bytes: the header as above with src = req.src and dst = the datagram's source; type, code, crc;
 * one 32-bit word -- 0 for types 1 and 3, long_be(req.arg) for type 4 --; the quote.  Types 1 and 3 are not
 * sent when the datagram's destination is multicast (first byte 0xff; the wrappers :229-293 return 0):
 * V_UNTOUCHED, nothing written.  Type 4 is sent regardless (:281-284).
 * Packet Too Big (type 2) -- documented difference (2) below: the layout of the other notices, the word =
 * long_be(req.arg), the MTU; code 0 whatever req.code says; the multicast rule of type 1.
 *   d_verdict[i]  ACCEPT = the answer is written and d_out_ans[i] set; V_UNTOUCHED as above; MALFORMED =
 *              nothing of the region is written: a descriptor past base_len or of fewer than 40 bytes, a
 *              req.type outside {0, 1, 2, 3, 4} or req.rsvd != 0, an echo record that fails the parse, a
 *              notice with q > desc.len, and -- for a record that would be answered -- a region past out_len
 *              or smaller than the answer.  For both d_out_ans[i] = {0, 0, 0}.
 * No byte outside a region is written, and inside it only the answer's own bytes.  Regions must not overlap.
 * Documented differences from the reference: (1) the reference takes an echo's T from the frame's length
 * (:110), so bytes behind the datagram (padding, a trailer) are echoed; the batch stops at the datagram's
 * end, as the ICMPv4 batch does.  (2) pico_icmp6_pkt_too_big calls pico_icmp6_notify with a type its switch
 * does not handle (:217-218, :271), so the reference sends nothing; the batch states the evident intent, as
 * the ICMPv4 batch does for options.
 * Out of scope: neighbour advertisements are not built (the reference harness captures none; a later
 * addition can take them as type 136); rate limiting, the route lookup and the choice of records stay with
 * the host.
 * Host checks, -EINVAL before any launch: a NULL required pointer (all but d_out_ans); d_desc, d_out_desc or
 * d_out_ans not 16-byte aligned; d_req not 4-byte aligned; flags != 0 (reserved).  n == 0 is a no-op;
 * without a device -ENODEV.  Two launches on one stream (verdicts; one wave per two records for the answers,
 * per record when base_len >= 1024 n), no allocation, no library scratch, no spin-wait, no host
 * synchronisation: capturable behind the batch whose verdicts chose the records.  Results never depend on
 * the launch shape. */
struct pico_csum_icmp6_req {   /* 24 bytes, per record, host-filled */
    uint8_t  src[16];          /* the answer's source where the rules above call for it */
    uint32_t arg;              /* host order: type 4 the pointer, type 2 the MTU; not read for 0 / 1 / 3 */
    uint8_t  type, code;       /* type 0: answer as pico_icmp6_process_in does (echo); 1 / 2 / 3 / 4: the notice */
    uint8_t  hop;              /* the answer's hop limit: the device's hostvars.hoplimit */
    uint8_t  rsvd;             /* must be 0 */
};
int pico_icmp6_reply_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc, uint32_t n,
                               const struct pico_csum_icmp6_req *d_req,
                               void *d_out, uint64_t out_len, const struct pico_csum_desc *d_out_desc,
                               struct pico_csum_desc *d_out_ans, uint8_t *d_verdict, uint32_t flags, void *stream);

/* Flow grouping: a verified burst, in arrival order, becomes the inputs of the three gather batches above
 * -- each flow's frames contiguous, in arrival order, and the groups[] over them -- on the device, with no
 * host pass per frame.  The batch form of the reference's per-frame lookups: pico_socket_tcp_deliver
 * (modules/pico_socket_tcp.c:125-226) walks the port's sockets comparing remote port, remote address and
 * local address; the fragment code compares id, source and destination (modules/pico_fragments.c:104-122,
 * :160-178, :447, :523).  A grouping by key equality: a parse, a hash table and a stable sort.
 *   d_desc[]   one frame each: desc.off -> the network header, desc.len = bytes available from there; with
 *              PICO_CSUM_FLOW_F_ETH desc.off -> the Ethernet header and the network header is 14 bytes on
 *              (the Ethernet batch's descriptors as they are).  desc.seed is not read.
 *   d_verdict_in  NULL, or the verdict array the Ethernet / IPv4 / IPv6 RX batch wrote for these frames
 *   mode_flags one of PICO_CSUM_FLOW_TCP / _FRAG4 / _FRAG6, | PICO_CSUM_FLOW_F_ETH
 * Selection.  A frame takes part when its region lies inside base_len (with F_ETH: and holds the 14
 * bytes), when, with d_verdict_in, its verdict with V_IPV6 masked off is V_ACCEPT (TCP mode) or V_FRAG
 * (the FRAG modes), and when it parses:
 *   TCP    IPv4: version 4, IHL >= 5, proto 6, neither MF nor an offset, the 4 port bytes at 4 IHL inside
 *          desc.len; IPv6: version 6, nxthdr 6 directly behind the fixed header (what the coalescing batch
 *          accepts), 44 bytes inside desc.len.  Key: family, src, dst, sport, dport.
 *   FRAG4  version 4, IHL >= 5, 20 bytes inside desc.len, MF or an offset.  Key: src, dst, id (bytes 4-5).
 *   FRAG6  version 6 and the extension-header walk of pico_ipv6_reassemble_batch_dev reaches the transport
 *          behind a fragment header whose 8 bytes lie inside desc.len.  Key: src, dst, that header's
 *          32-bit id.
 * Nothing past desc.len or base_len contributes; reads follow the whole-16-byte-block rule above.
 * Groups.  Two selected frames are in one group exactly when their keys are equal.  In TCP mode the first
 * n_known groups are the host's connection table: group t < n_known is d_known[t]'s (compared field by
 * field: family, all 16 bytes of src and of dst, sport, dport; reserved is not compared), possibly empty;
 * a table key equal to an earlier one gets an empty group.  Groups of keys not in the table follow in order
 * of their first arrival.  n_known must be 0 in the FRAG modes.  Members of a group are in arrival order
 * (ascending input index).
 *   d_out_groups[2g], [2g+1]  the group's first slot and count (uint32[2 (n + n_known)]); an empty table
 *              group and every entry from n_groups up to n + n_known are {0, 0}
 *   d_out_desc[slot]   {network header offset, bytes available from there, 0}: with F_ETH {off + 14,
 *              len - 14, 0}, else {off, len, 0}
 *   d_out_index[slot]  the frame's input index.  Slots past the selected frames hold {0, 0, 0} and the
 *              unselected input indexes in ascending order: d_out_index is a permutation of 0 .. n-1
 *   d_out_counts[0]    n_groups (the n_known table groups included);  [1] the number of selected frames
 * d_out_desc and d_out_groups go to pico_ipv4_reassemble_batch_dev, pico_ipv6_reassemble_batch_dev and
 * pico_tcp_coalesce_batch_dev as they are (n_frag / n_seg = n; n_dgram / n_conn = n_groups, or a fixed cap:
 * a padded or empty group is those batches' "empty group" -- MALFORMED, nothing written).  Table groups
 * keep table order, so the host's per-connection d_conn[] / d_out_desc[] line up with no round trip; the
 * host reads back only d_out_counts and, for the groups >= n_known, d_out_index[first]: that leader's
 * frame holds the new flow's tuple.
 * One documented difference: the reference matches a socket bound to INADDR_ANY against any destination;
 * the batch groups by exact destination.  Two groups that resolve to one socket are the host's to merge.
 * Errors, all checked on the host before any launch, -EINVAL: n == 0 or n + n_known > 0x00FFFFFF; an
 * unknown mode or flag; n_known != 0 in a FRAG mode; d_known == NULL with n_known != 0; a NULL d_base,
 * d_desc, d_out_desc, d_out_index, d_out_groups, d_out_counts or d_scratch; d_desc, d_out_desc or d_scratch
 * not 16-byte aligned; scratch_len < pico_flow_group_scratch_bytes(n, n_known) (pure host arithmetic; 0 =
 * out of range; never smaller for a larger n or n_known).  No usable device: -ENODEV.
 * Results never depend on hash_seed (it exists so that a host can make hash collisions unpredictable to a
 * sender, as an RSS key does), on the scratch contents on entry, or on the launch shape.  Everything runs
 * on `stream`: no allocation, no host synchronisation, no library scratch -- the caller's d_scratch holds
 * everything, and the batch initialises on the stream what it needs of it.  The number of launches
 * depends only on n and n_known, so a call is capturable into a graph as a straight line, together with
 * the gather batch behind it.  Every device loop is bounded by a value known on entry and no lane waits
 * for another lane's store. */
struct pico_csum_flow_key {      /* 40 bytes */
    uint8_t  src[16];            /* the frame's source address as stored; IPv4: bytes 0-3, rest 0 */
    uint8_t  dst[16];            /* the frame's destination address, likewise */
    uint16_t sport, dport;       /* TCP ports as stored (network byte order) */
    uint8_t  family;             /* 4 or 6 */
    uint8_t  reserved[3];        /* 0 */
};
#define PICO_CSUM_FLOW_TCP   1u  /* key: family, src, dst, sport, dport */
#define PICO_CSUM_FLOW_FRAG4 2u  /* key: src, dst, id (header bytes 4-5) */
#define PICO_CSUM_FLOW_FRAG6 3u  /* key: src, dst, the fragment header's 32-bit id */
#define PICO_CSUM_FLOW_F_ETH 0x10u /* desc.off -> the Ethernet header; the network header is 14 bytes on */

uint64_t pico_flow_group_scratch_bytes(uint32_t n, uint32_t n_known);   /* pure host arithmetic; 0 = out of range */

int pico_flow_group_batch_dev(const void *d_base, uint64_t base_len, const struct pico_csum_desc *d_desc, uint32_t n,
                              const uint8_t *d_verdict_in, uint32_t mode_flags,
                              const struct pico_csum_flow_key *d_known, uint32_t n_known, uint32_t hash_seed,
                              struct pico_csum_desc *d_out_desc, uint32_t *d_out_index, uint32_t *d_out_groups,
                              uint32_t *d_out_counts, void *d_scratch, uint64_t scratch_len, void *stream);

/* ---------------------------------------------------------------- layer 3 */

struct pico_csum_ctx;  /* device, three streams and staging slots (the uniform ring alternates two;
                         * staged descriptor batches rotate over three, the third staging buffer
                         * allocated on their first call) */

struct pico_csum_ctx *pico_csum_ctx_create(int device, uint64_t staging_bytes);
void pico_csum_ctx_destroy(struct pico_csum_ctx *ctx);

/* Host-resident uniform batch: frames in host memory (pinned for full PCIe
 * rate, see pico_csum_host_register), results to host memory; returns when
 * d2h of every result has completed. */
int pico_checksum_batch_uniform_host(struct pico_csum_ctx *ctx, const void *base, uint64_t stride,
                                     uint32_t len, uint32_t n, uint32_t seed, uint16_t *out);
/* Host-resident descriptor batches: the TAP / pico_device burst as the stack holds it
 * (frames anywhere in `base`, base_len bytes, descriptors and results in host memory; pin
 * `base` and the outputs with pico_csum_host_register for full PCIe rate).  Consecutive
 * descriptors whose bytes span at most the ctx staging size form a chunk: the span and the
 * rebased descriptors go H2D, the device batch of the same name runs, and only the per-frame
 * results come back (with PICO_CSUM_F_WRITE also the span, crc fields stored); chunk c+1's
 * H2D overlaps chunk c's kernel and D2H on the other stream.  Results, verdicts and error
 * rules are those of the _dev functions; on the staged path a frame larger than the staging
 * buffer is -EINVAL.  With F_WRITE, frames of different chunks must not share bytes (true for a
 * frame ring).  A burst the device addresses directly (page-locked) is read in place instead:
 * pico_csum_set_host_in_place.  Returns when every result is in host memory. */
int pico_checksum_batch_host(struct pico_csum_ctx *ctx, const void *base, uint64_t base_len,
                             const struct pico_csum_desc *desc, uint32_t n, int32_t crc_off, uint32_t flags,
                             uint16_t *out);
int pico_ipv4_checksum_batch_host(struct pico_csum_ctx *ctx, const void *base, uint64_t base_len,
                                  const struct pico_csum_desc *desc, uint32_t n, uint32_t flags, uint16_t *out_net,
                                  uint16_t *out_transport, uint8_t *verdict);
int pico_ipv6_checksum_batch_host(struct pico_csum_ctx *ctx, const void *base, uint64_t base_len,
                                  const struct pico_csum_desc *desc, uint32_t n, uint32_t flags,
                                  uint16_t *out_transport, uint8_t *verdict);
int pico_eth_checksum_batch_host(struct pico_csum_ctx *ctx, const void *base, uint64_t base_len,
                                 const struct pico_csum_desc *desc, uint32_t n, uint32_t flags, const uint8_t *mac,
                                 uint16_t *out_net, uint16_t *out_transport, uint8_t *verdict);
int pico_csum_host_register(void *ptr, uint64_t bytes);
int pico_csum_host_unregister(void *ptr);
/* Zero-copy ingress (the batch form of pico_stack_recv_zerocopy, stack/pico_stack.c:479-527: the
 * driver's buffer is used where it lies): the device's address of registered host memory (NULL and
 * pico_csum_last_error() if ptr is not registered).  Any layer-2 batch takes it as d_base -- and as
 * d_desc / the outputs, registered the same way -- and the kernel then reads the frames over PCIe in
 * place, with no staging copy. */
void *pico_csum_host_device_pointer(void *ptr);

/* ---------------------------------------------------------------- misc */

int pico_csum_abi_version(void);
const char *pico_csum_last_error(void);   /* thread-local, "" when none */

/* Launch-shape override for tests and bench sweeps (all 0 = automatic choice); applies to
 * launches from the calling thread only (thread-local).
 *   group 2: descriptor batches (the sorted-rounds kernel) with fpw frames per wave (1..64);
 *            the other arguments are ignored.
 *   group 4..64 (power of 2): uniform rings -- lanes per frame; cpl = 16-byte chunks per lane
 *            per pass (1,2,4,8; 3 and 5-7 with group >= 8 and pipeline != 1: the pipelined
 *            kernel, frames past its one pass round cpl up to 4 / 8); unroll = frames in flight per group (1,2,4; cpl*unroll <= 8);
 *            fpw = frames per wave (multiple of 64/group, <= 64); nt = 0 auto / 1 plain /
 *            2 non-temporal loads; pipeline = 0 auto / 1 off / 2 on / 3 on with global instead
 *            of buffer-window loads (frames that fit one pass: double-buffered frame sets).
 * A group for the other batch kind makes the batch call return -EINVAL. */
int pico_csum_set_launch_override(uint32_t group, uint32_t cpl, uint32_t unroll, uint32_t fpw, uint32_t nt,
                                  uint32_t pipeline);

/* Host-resident descriptor batches (pico_*_batch_host), per calling thread: 1 (the default) = a
 * burst whose whole [base, base + base_len) the device addresses directly -- page-locked by
 * hipHostMalloc or pico_csum_host_register -- is read (and with F_WRITE written) in place by the
 * kernel, only descriptors and results staged, and nothing staged when the descriptor and result
 * arrays are device-addressable too (then frames larger than the staging buffer are fine);
 * 0 = always through the staging buffers.  Results never depend on it. */
int pico_csum_set_host_in_place(uint32_t on);

/* Tuning knob (tests / bench sweeps), per calling thread: the uniform rings' stream waves
 * (pico_checksum_batch_uniform_dev / _host on densely packed frames) -- mode 0 = automatic, 1 = on
 * wherever the ring allows them, PICO_CSUM_STREAM_OFF = the lane-group kernels; frames_per_wave
 * 0 = automatic.  Results never depend on it. */
#define PICO_CSUM_STREAM_OFF 0xFFu
int pico_csum_set_uniform_stream(uint32_t mode, uint32_t frames_per_wave);

/* Tuning knob (tests / bench sweeps), per calling thread: the reassembly batches' flat grid
 * (pico_ipv4_reassemble_batch_dev / pico_ipv6_reassemble_batch_dev) -- 0 = automatic (batches
 * of 512 datagrams or more), 1 = always, 2 = never (one workgroup per datagram).  Results never
 * depend on it. */
int pico_csum_set_reasm_flat(uint32_t mode);

/* Frees the calling thread's reassembly scratch (the flat grid's tallies, one buffer per stream
 * the thread launched on) and the scratch of captured graphs destroyed since; the thread's next
 * flat-grid call allocates again.  A thread's scratch is also freed when the thread exits.  Call
 * it with no reassembly of this thread still running on the device (hipFree waits for the device).
 * Returns 0, or -PICO_CSUM_ENODEV without a device. */
int pico_csum_release_thread_scratch(void);

#ifdef __cplusplus
}
#endif
#endif /* PICO_CSUM_H */
