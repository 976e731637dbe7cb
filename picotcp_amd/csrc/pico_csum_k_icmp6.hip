// pico_csum_k_icmp6.hip -- a burst's ICMPv6 answers: echo replies (the request's transport copied and
// summed in one pass, the pseudo header seeded) and the notices of pico_icmp6_notify (destination
// unreachable, packet too big, time exceeded, parameter problem: up to 1232 quoted bytes, copied and
// summed the same way), each a finished IPv6 datagram in its own output region -- and its launcher.
// The contract: include/pico_csum.h, pico_icmp6_reply_batch_dev.  Helpers, the extension-header walk
// (ipv6_walk_packed), the 16-byte unit mover (unit_pair_move), the header word's halves and store
// (halves, store_word) and the arithmetic contract: pico_csum_dev.h.
//
// Reference: pico_icmp6_process_in / pico_icmp6_send_echoreply (modules/pico_icmp6.c:94-133, :61-92: a
// fresh frame, type 129, code 0, id / seq and the payload copied, pico_icmp6_checksum :38-55 over the
// pseudo header and the transport); pico_ipv6_frame_push (modules/pico_ipv6.c:1324-1339, the header
// :1283-1322: 60 00 00 00, len, nxthdr, the device's hop limit, a multicast source replaced by the
// link's address); pico_icmp6_notify (modules/pico_icmp6.c:153-227: min(40 + len field, 1232) bytes
// quoted behind type, code, crc and one 32-bit word) and its wrappers (:229-293: nothing towards a
// multicast destination, but for the parameter problem).  The reference keeps no state for ICMPv6.
//
// Two launches on one stream (K13's first and third; there is no duplicate rule here):
//   K14a  one lane per record: every check, the extension-header walk -> verdict ACCEPT / UNTOUCHED /
//         MALFORMED and the answer's descriptor.
//   K14b  one wave per two records, the unit mover's two members (or per record: K13's launch shapes
//         and its threshold, below).  Lanes 0-11 hold the answer's IPv6 header and the 8 bytes behind
//         it (type, code, crc; an echo's id / seq, a notice's word), a notice's lanes 12-15 the
//         quote's first 16 bytes.  The mover carries the rest -- an echo's transport bytes 8 .. T to
//         d + 48, a notice's quote bytes 16 .. q to d + 64 -- into its member's sum (SPLIT), which
//         starts with the pseudo header and the lanes' own words.  A notice's quote begins at the
//         descriptor's first byte, and the mover's first load may start up to 15 bytes before its
//         source: with 16 quoted bytes on the lanes that load stays inside the datagram.  Behind the
//         wave's two reductions the lanes' words are written once, complete (store_word).  Nothing is
//         stored for a record that is not ACCEPT.
#include "pico_csum_dev.h"

namespace {

struct Icmp6Args {
    const uint8_t* base;
    uint64_t base_len;
    const pico_csum_desc_dev* desc;
    uint32_t n;
    const uint32_t* req;                // struct pico_csum_icmp6_req as six words: src[4]; arg; type | code << 8 | hop << 16 | rsvd << 24
    uint8_t* out;
    uint64_t out_len;
    const pico_csum_desc_dev* odesc;
    pico_csum_desc_dev* o_ans;
    uint8_t* verdict;
};
constexpr uint32_t ICMP6_QUOTE_MAX = 1232u;   // PICO_IPV6_MIN_MTU 1280 - the IPv6 header - the ICMPv6 header's 8

// An echo request's transport offset: the datagram's 40 + plen bytes walked (next header 58 at once:
// no walk).  WALK_PROTO with proto 58: net_len; everything else as the walk says.
__device__ __forceinline__ int icmp6_walk(const uint8_t* h, uint32_t plen, uint32_t& net_len, uint32_t& proto) {
    net_len = 40u;
    proto = h[6];
    if (proto == 58u) return WALK_PROTO;
    const uint64_t r = ipv6_walk_packed(h, 40u + plen);
    net_len = (uint32_t)(r >> 8) & 0xFFFFu;
    proto = (uint32_t)(r >> 24) & 0xFFu;
    return (int)(r & 0xFFu) - 1;
}

// Every check of record i, in an order that never reads past desc.len; alen = the answer's bytes
// (0 unless ACCEPT).
__device__ __forceinline__ uint32_t icmp6_judge(const Icmp6Args& p, uint64_t i, uint32_t& alen) {
    alen = 0;
    const pico_csum_desc_dev d = p.desc[i], od = p.odesc[i];
    const uint32_t r5 = p.req[6u * i + 5u], type = r5 & 0xFFu;
    if (span_out(d, p.base_len) || d.len < 40u) return V_MALFORMED;
    if (type > 4u || (r5 >> 24) != 0u) return V_MALFORMED;
    const uint8_t* h = p.base + d.off;
    const uint32_t plen = bswap16(ld32(h + 4) & 0xFFFFu);
    uint32_t need;
    if (type == 0u) {
        if (((uint32_t)h[0] >> 4) != 6u || 40u + plen > d.len) return V_MALFORMED;
        uint32_t net_len, proto;
        const int kind = icmp6_walk(h, plen, net_len, proto);
        if (kind == WALK_BAD) return V_MALFORMED;
        if (kind != WALK_PROTO || proto != 58u) return V_UNTOUCHED;      // discarded, a fragment, another protocol
        if (net_len + 8u > 40u + plen) return V_MALFORMED;
        if ((uint32_t)h[net_len] != 128u) return V_UNTOUCHED;            // ND, MLD, replies, errors: the host's
        need = 40u + (40u + plen - net_len);
    } else {
        if (type != 4u && (uint32_t)h[24] == 0xFFu) return V_UNTOUCHED;  // the wrappers: nothing towards a multicast destination
        const uint32_t q = min(40u + plen, ICMP6_QUOTE_MAX);
        if (q > d.len) return V_MALFORMED;
        need = 48u + q;
    }
    if (span_out(od, p.out_len) || need > od.len) return V_MALFORMED;
    alen = need;
    return V_ACCEPT;
}

__global__ __launch_bounds__(256) void icmp6_verdict_kernel(Icmp6Args p) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    uint32_t alen;
    const uint32_t v = icmp6_judge(p, i, alen);
    p.verdict[i] = (uint8_t)v;
    if (p.o_ans) p.o_ans[i] = pico_csum_desc_dev{alen ? p.odesc[i].off : 0u, alen, 0u};
}

// One record of a wave's pair (every field wave-uniform).  on: an answer is written.  The mover's
// part: pl bytes from s to d + 4 nw, e = the end of the datagram's last readable block.
struct Icmp6Member {
    bool on, echo, own_src;
    const uint8_t* h;       // the answered datagram's IPv6 header
    const uint32_t* r;      // its request record
    uint64_t d;             // the answer
    uint64_t s, e;
    uint32_t pl, nw;        // moved bytes; the words the lanes hold (12: an echo, 16: a notice)
    uint32_t toff;          // an echo request's transport offset
    uint32_t w1;            // the header's second word: len, nxthdr 58, hop
    uint32_t icmp0, word;   // type | code << 8 (crc 0); a notice's 32-bit word as stored
    uint32_t pseudo;        // long_be(upper-layer length) and nxthdr 58 of the pseudo header, as halves
};

__device__ __forceinline__ Icmp6Member icmp6_member(const Icmp6Args& p, uint64_t i, bool exists) {
    Icmp6Member m{};
    if (!exists || uni((uint32_t)p.verdict[i]) != V_ACCEPT) return m;
    const uint64_t off = uni64(p.desc[i].off), ooff = uni64(p.odesc[i].off);
    const uint32_t dlen = uni(p.desc[i].len);
    m.r = p.req + 6u * i;
    const uint32_t arg = uni(m.r[4]), r5 = uni(m.r[5]), type = r5 & 0xFFu;
    m.on = true;
    m.echo = type == 0u;
    m.h = p.base + off;
    m.d = reinterpret_cast<uint64_t>(p.out) + ooff;
    m.e = (reinterpret_cast<uint64_t>(m.h) + dlen + 15u) & ~(uint64_t)15;
    const uint32_t plen = bswap16(uni(ld32(m.h + 4)) & 0xFFFFu);
    uint32_t L;                                                      // the answer's transport bytes
    if (m.echo) {
        uint32_t proto;
        icmp6_walk(m.h, plen, m.toff, proto);
        m.toff = uni(m.toff);
        L = 40u + plen - m.toff;
        m.nw = 12u;
        m.pl = L - 8u;
        m.s = reinterpret_cast<uint64_t>(m.h) + m.toff + 8u;
        m.own_src = uni((uint32_t)m.h[24]) != 0xFFu;                 // ipv6_push_hdr_adjust: a multicast source -> the link's
        m.icmp0 = 129u;
    } else {
        const uint32_t q = min(40u + plen, ICMP6_QUOTE_MAX);
        L = 8u + q;
        m.nw = 16u;
        m.pl = q - 16u;
        m.s = reinterpret_cast<uint64_t>(m.h) + 16u;
        m.icmp0 = type | (type == 2u ? 0u : ((r5 >> 8) & 0xFFu) << 8);
        m.word = type == 2u || type == 4u ? __builtin_bswap32(arg) : 0u;
    }
    m.w1 = bswap16(L) | (58u << 16) | (((r5 >> 16) & 0xFFu) << 24);
    m.pseudo = bswap16(L) + (58u << 8);
    return m;
}

// The lane's word of the member's first 4 nw bytes (ICMPv6 crc 0); lane < m.nw.  Words 0-1: 60 00 00 00,
// len, 58, hop; 2-5: the source (an echo: the request's destination, unless multicast; else req.src);
// 6-9: the datagram's source; 10: type, code, crc; 11: an echo's id / seq, a notice's word; a notice's
// 12-15: the quote's first 16 bytes.
__device__ __forceinline__ uint32_t icmp6_word(const Icmp6Member& m, uint32_t lane) {
    if (lane == 0u) return 0x60u;
    if (lane == 1u) return m.w1;
    if (lane < 6u) return m.echo && m.own_src ? ld32(m.h + 24u + 4u * (lane - 2u)) : m.r[lane - 2u];
    if (lane < 10u) return ld32(m.h + 8u + 4u * (lane - 6u));
    if (lane == 10u) return m.icmp0;
    if (lane == 11u) return m.echo ? ld32(m.h + m.toff + 4u) : m.word;
    return ld32(m.h + 4u * (lane - 12u));
}

// Launch shapes: K13's (pico_csum_k_icmp.hip) -- a wave takes two records (PAIR), or, in batches whose
// datagrams average ICMP6_LONE_AVG bytes or more, one, member B void.  The threshold is K13's 1024, which
// was never measured itself; it is taken over as it stands.  Results never depend on the shape.
constexpr uint64_t ICMP6_LONE_AVG = 1024u;

template <uint32_t ICMP6_U, bool PAIR>
__global__ __launch_bounds__(256) void icmp6_answer_kernel(Icmp6Args p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = uni64((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint64_t iA = PAIR ? 2u * w : w, iB = iA + 1u;
    if (iA >= p.n) return;
    const Icmp6Member A = icmp6_member(p, iA, true), B = icmp6_member(p, iB, PAIR && iB < p.n);
    if (!A.on && !B.on) return;

    const bool hA = A.on && lane < A.nw, hB = B.on && lane < B.nw;
    const uint32_t wA = hA ? icmp6_word(A, lane) : 0u, wB = hB ? icmp6_word(B, lane) : 0u;
    // pico_icmp6_checksum: the pseudo header (the addresses are the header's words 2-9; the length and
    // the next header on lane 0), the lanes' transport words, and the rest as the mover copies it
    uint32_t accA = (hA && lane >= 2u ? halves(wA) : 0u) + (hA && lane == 0u ? A.pseudo : 0u);
    uint32_t accB = (hB && lane >= 2u ? halves(wB) : 0u) + (hB && lane == 0u ? B.pseudo : 0u);
    unit_pair_move<ICMP6_U, false, true>(A.s, B.s, A.on ? A.d + 4u * A.nw : 0u, B.on ? B.d + 4u * B.nw : 0u, A.e, B.e, A.pl,
                                         B.pl, B.on, lane, accA, accB);
    const uint32_t crcA = finalize(wave_total(accA));
    const uint32_t crcB = finalize(wave_total(accB));

#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (!(b ? hB : hA)) continue;
        uint32_t v = b ? wB : wA;
        if (lane == 10u) v |= bswap16(b ? crcB : crcA) << 16;
        store_word(reinterpret_cast<uint8_t*>(b ? B.d : A.d) + 4u * lane, v);
    }
}

}  // namespace

extern "C" {

int pico_csum_launch_icmp6_reply(const void* base, uint64_t base_len, const void* desc, uint32_t n, const void* req,
                                 void* out, uint64_t out_len, const void* out_desc, void* o_ans, uint8_t* verdict,
                                 void* stream) {
    if (n == 0) return (int)hipSuccess;
    if (!verdict) return (int)hipErrorInvalidValue;
    Icmp6Args a{static_cast<const uint8_t*>(base), base_len, static_cast<const pico_csum_desc_dev*>(desc), n,
                static_cast<const uint32_t*>(req), static_cast<uint8_t*>(out), out_len,
                static_cast<const pico_csum_desc_dev*>(out_desc), static_cast<pico_csum_desc_dev*>(o_ans), verdict};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(256);
    const uint64_t pairs = ((uint64_t)n + 1u) / 2u;
    hipLaunchKernelGGL(icmp6_verdict_kernel, dim3((unsigned)(((uint64_t)n + 255u) / 256u)), block, 0, s, a);
    if (base_len >= ICMP6_LONE_AVG * n)
        hipLaunchKernelGGL((icmp6_answer_kernel<3u, false>), dim3((unsigned)(((uint64_t)n + 3u) / 4u)), block, 0, s, a);
    else
        hipLaunchKernelGGL((icmp6_answer_kernel<3u, true>), dim3((unsigned)((pairs + 3u) / 4u)), block, 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"
