// pico_csum_k_icmp.hip -- a burst's ICMPv4 answers: echo replies (the request's transport copied
// and summed in one pass) and the notices of pico_icmp4_notify (unreachable, time exceeded,
// parameter problem), each a finished IPv4 datagram in its own output region -- and its launcher.
// The contract: include/pico_csum.h, pico_icmp4_reply_batch_dev.  Helpers, the 16-byte unit mover
// (unit_pair_move), the header word's halves and store (halves, store_word) and the arithmetic
// contract: pico_csum_dev.h.
//
// Reference: pico_icmp4_process_in (modules/pico_icmp4.c:47-85: type 8 -> 0, the duplicate check on
// its statics :61-69, pico_icmp4_checksum :30-41 over the whole transport, pico_ipv4_rebound);
// pico_ipv4_rebound / pico_ipv4_frame_push (modules/pico_ipv4.c:1512-1533, :1039-1079: vhl 45, len,
// id, the frame's own frag :1072-1075, ttl, proto, pico_ipv4_checksum); pico_icmp4_notify
// (modules/pico_icmp4.c:106-141: min(len field, 28) bytes quoted behind type, code, crc, 00 00,
// nmtu 1500).
//
// Four launches on one stream (K5's pattern, pico_csum_k_sorted.hip, with the mover between):
//   K13a  one lane per record: every check -> verdict ACCEPT / UNTOUCHED / MALFORMED and the
//         answer's descriptor.
//   K13b  one lane per record: an ACCEPT echo request's nearest earlier echo request (a wave
//         ballot, the workgroup's wave maxima in LDS, then -- for the workgroup's first one only -- a
//         backward scan over the earlier verdict bytes, 256 a step); equal (id, seq): DUPLICATE, its
//         descriptor zeroed.  Bytes another workgroup turns from ACCEPT to DUPLICATE meanwhile count
//         the same (both are echo requests).
//   K13c  one wave per two records, the unit mover's two members (or per record: the launch shapes
//         below): an echo's transport bytes 4 .. T move through unit_pair_move into their own
//         member's sum (SPLIT); a notice's quote is one 32-bit word a lane.  Behind the wave's two reductions each answer's header words -- the
//         IPv4 header, the ICMP header with its checksum, a notice's quote -- are written once,
//         complete (store_word).  Nothing is stored for a record that is not ACCEPT.
//   K13d  one workgroup: the batch's last echo request's (id, seq) -> the carried state.
#include "pico_csum_dev.h"

namespace {

struct Icmp4Args {
    const uint8_t* base;
    uint64_t base_len;
    const pico_csum_desc_dev* desc;
    uint32_t n;
    const uint32_t* req;                // struct pico_csum_icmp4_req as two words: src; id | type << 16 | code << 24
    uint32_t* state;                    // struct pico_csum_icmp4_state as two words: seen; id | seq << 16 (as stored)
    uint8_t* out;
    uint64_t out_len;
    const pico_csum_desc_dev* odesc;
    pico_csum_desc_dev* o_ans;
    uint8_t* verdict;
};
constexpr uint32_t V_DUPLICATE = 64u;   // the forwarding batch's bit (include/pico_csum.h)

__device__ __forceinline__ uint32_t req_type(const Icmp4Args& p, uint64_t i) { return (p.req[2u * i + 1u] >> 16) & 0xFFu; }

// Every check of record i, in an order that never reads past desc.len; alen = the answer's bytes
// (0 unless ACCEPT).
__device__ __forceinline__ uint32_t icmp4_judge(const Icmp4Args& p, uint64_t i, uint32_t& alen) {
    alen = 0;
    const pico_csum_desc_dev d = p.desc[i], od = p.odesc[i];
    const uint32_t type = req_type(p, i);
    if (span_out(d, p.base_len) || d.len < 20u) return V_MALFORMED;
    if (!(type == 0u || type == 3u || type == 11u || type == 12u)) return V_MALFORMED;
    const uint8_t* h = p.base + d.off;
    const uint32_t w0 = ld32(h), tot = bswap16(w0 >> 16);
    uint32_t need;
    if (type == 0u) {
        const uint32_t ihl = w0 & 15u, hl = 4u * ihl;
        if (((w0 >> 4) & 15u) != 4u || ihl < 5u || (uint32_t)h[9] != 1u) return V_MALFORMED;
        if (tot < hl + 8u || tot > d.len) return V_MALFORMED;
        if ((uint32_t)h[hl] != 8u) return V_UNTOUCHED;
        need = 20u + tot - hl;
    } else {
        const uint32_t q = min(tot, 28u);
        if (tot < 20u || q > d.len) return V_MALFORMED;
        need = 28u + q;
    }
    if (span_out(od, p.out_len) || need > od.len) return V_MALFORMED;
    alen = need;
    return V_ACCEPT;
}

__global__ __launch_bounds__(256) void icmp4_verdict_kernel(Icmp4Args p) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    uint32_t alen;
    const uint32_t v = icmp4_judge(p, i, alen);
    p.verdict[i] = (uint8_t)v;
    if (p.o_ans) p.o_ans[i] = pico_csum_desc_dev{alen ? p.odesc[i].off : 0u, alen, 0u};
}

// an echo request that reached the duplicate check
__device__ __forceinline__ bool echo_reached(const Icmp4Args& p, uint64_t j) {
    const uint32_t v = p.verdict[j];
    return (v == V_ACCEPT || v == V_DUPLICATE) && req_type(p, j) == 0u;
}

// (id, seq) of echo request j as stored: the ICMP header's second word
__device__ __forceinline__ uint32_t echo_idseq(const Icmp4Args& p, uint64_t j) {
    const uint8_t* h = p.base + p.desc[j].off;
    return ld32(h + 4u * ((uint32_t)h[0] & 15u) + 4u);
}

// The highest index < below (a multiple of 256) that is an echo request, or -1: the whole workgroup
// scans backwards 256 records a step.
__device__ __forceinline__ int64_t echo_scan_back(const Icmp4Args& p, uint64_t below, int* wmax) {
    const uint32_t t = threadIdx.x, w = t >> 6;
    for (uint64_t top = below; top != 0; top -= 256u) {
        const bool e = echo_reached(p, top - 256u + t);
        const uint64_t b = __builtin_amdgcn_ballot_w64(e);
        __syncthreads();
        if ((t & 63u) == 0) wmax[w] = b ? 63 - __builtin_clzll(b) + 64 * (int)w : -1;
        __syncthreads();
        const int m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        if (m >= 0) return (int64_t)(top - 256u) + m;
    }
    return -1;
}

__global__ __launch_bounds__(256) void icmp4_dup_kernel(Icmp4Args p) {
    __shared__ int wlast[4], wmax[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint64_t blk0 = (uint64_t)blockIdx.x * 256u, i = blk0 + t;
    const bool elig = i < p.n && p.verdict[i] == V_ACCEPT && req_type(p, i) == 0u;   // DUPLICATE is written only after the reads below
    const uint64_t b = __builtin_amdgcn_ballot_w64(elig);
    if (lane == 0) wlast[w] = b ? 63 - __builtin_clzll(b) : -1;
    __syncthreads();
    int64_t prev = -1;
    const uint64_t below = b & ((1ull << lane) - 1ull);
    if (below) {
        prev = (int64_t)(blk0 + 64u * w + 63u - __builtin_clzll(below));
    } else {
        for (int k = (int)w - 1; k >= 0; --k)
            if (wlast[k] >= 0) { prev = (int64_t)(blk0 + 64u * k + wlast[k]); break; }
    }
    // the workgroup's first echo request looks further back (workgroup-uniform condition)
    const bool any = wlast[0] >= 0 || wlast[1] >= 0 || wlast[2] >= 0 || wlast[3] >= 0;
    int64_t back = -1;
    if (any && blk0 != 0) back = echo_scan_back(p, blk0, wmax);
    if (!elig) return;
    if (prev < 0) prev = back;
    bool have = false;
    uint32_t last = 0;
    if (prev >= 0) {
        have = true;
        last = echo_idseq(p, (uint64_t)prev);
    } else if (p.state) {                                           // :61 !firstpkt
        have = p.state[0] != 0u;
        last = p.state[1];
    }
    if (have && echo_idseq(p, i) == last) {
        p.verdict[i] = (uint8_t)V_DUPLICATE;
        if (p.o_ans) p.o_ans[i] = pico_csum_desc_dev{0u, 0u, 0u};
    }
}

__global__ __launch_bounds__(256) void icmp4_state_kernel(Icmp4Args p) {
    __shared__ int wmax[4];
    const uint64_t top = ((uint64_t)p.n + 255u) & ~(uint64_t)255u;
    const uint32_t t = threadIdx.x, w = t >> 6;
    int64_t last = -1;
    {
        const uint64_t j = top - 256u + t;                           // records past n are not ours
        const bool e = j < p.n && echo_reached(p, j);
        const uint64_t b = __builtin_amdgcn_ballot_w64(e);
        if ((t & 63u) == 0) wmax[w] = b ? 63 - __builtin_clzll(b) + 64 * (int)w : -1;
        __syncthreads();
        const int m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        if (m >= 0) last = (int64_t)(top - 256u) + m;
    }
    if (last < 0 && top > 256u) last = echo_scan_back(p, top - 256u, wmax);
    if (last >= 0 && t == 0) {
        p.state[0] = 1u;
        p.state[1] = echo_idseq(p, (uint64_t)last);
    }
}

// One record of a wave's pair (every field wave-uniform).  on: an answer is written.  The mover's
// part (an echo): pl bytes from s to d + 24, e = the end of the request's last readable block.
struct Icmp4Member {
    bool on, echo;
    const uint8_t* h;       // the answered datagram's IPv4 header
    uint64_t d;             // the answer
    uint64_t s, e;
    uint32_t pl, q, nw;     // moved bytes; a notice's quoted bytes; the words written behind the reduction
    uint32_t ip[5];         // the answer's IPv4 header as little-endian words, crc set
    uint32_t icmp0;         // type | code << 8 (crc 0)
};

__device__ __forceinline__ Icmp4Member icmp4_member(const Icmp4Args& p, uint64_t i, bool exists) {
    Icmp4Member m{};
    if (!exists || uni((uint32_t)p.verdict[i]) != V_ACCEPT) return m;
    const uint64_t off = uni64(p.desc[i].off), ooff = uni64(p.odesc[i].off);
    const uint32_t dlen = uni(p.desc[i].len), r0 = uni(p.req[2u * i]), r1 = uni(p.req[2u * i + 1u]);
    const uint32_t type = (r1 >> 16) & 0xFFu;
    m.on = true;
    m.echo = type == 0u;
    m.h = p.base + off;
    m.d = reinterpret_cast<uint64_t>(p.out) + ooff;
    const uint32_t w0 = uni(ld32(m.h)), w1 = uni(ld32(m.h + 4)), tot = bswap16(w0 >> 16);
    uint32_t alen;
    if (m.echo) {
        const uint32_t hl = 4u * (w0 & 15u), T = tot - hl;
        alen = 20u + T;
        m.pl = T - 4u;
        m.s = reinterpret_cast<uint64_t>(m.h) + hl + 4u;
        m.e = (reinterpret_cast<uint64_t>(m.h) + dlen + 15u) & ~(uint64_t)15;
        m.nw = 6u;
        m.icmp0 = uni((uint32_t)m.h[hl + 1u]) << 8;                  // type 0, the request's code
    } else {
        m.q = min(tot, 28u);
        alen = 28u + m.q;
        m.nw = 7u + ((m.q + 3u) >> 2);
        m.icmp0 = type | ((r1 >> 24) << 8);
    }
    // pico_ipv4_frame_push: 45, tos 0, len; id, frag (an echo: the request's field as it lies, a
    // notice: 0); ttl 64, proto 1, crc; src; dst = the datagram's source
    m.ip[0] = 0x45u | (bswap16(alen) << 16);
    m.ip[1] = bswap16(r1 & 0xFFFFu) | (m.echo ? w1 & 0xFFFF0000u : 0u);
    m.ip[2] = 64u | (1u << 8);
    m.ip[3] = r0;
    m.ip[4] = uni(ld32(m.h + 12));
    const uint32_t crc = finalize(halves(m.ip[0]) + halves(m.ip[1]) + halves(m.ip[2]) + halves(m.ip[3]) + halves(m.ip[4]));
    m.ip[2] |= bswap16(crc) << 16;
    return m;
}

// The lane's word of the member's header words (ICMP crc 0) and how many of its bytes belong to the
// answer (0: none).  Words 0-4: the IPv4 header; 5: type, code, crc; a notice's 6: 00 00 05 dc
// (ipm_void, ipm_nmtu = 1500), 7 ..: the quote, the last word up to three bytes short.
__device__ __forceinline__ uint32_t icmp4_word(const Icmp4Member& m, uint32_t lane, uint32_t& nb) {
    nb = m.on && lane < m.nw ? 4u : 0u;
    if (nb == 0u) return 0u;
    if (lane < 5u) return lane == 0u ? m.ip[0] : lane == 1u ? m.ip[1] : lane == 2u ? m.ip[2] : lane == 3u ? m.ip[3] : m.ip[4];
    if (lane == 5u) return m.icmp0;
    if (lane == 6u) return 0xDC050000u;
    const uint32_t k = 4u * (lane - 7u);
    nb = min(4u, m.q - k);
    if (nb == 4u) return ld32(m.h + k);
    uint32_t w = 0;
    for (uint32_t b = 0; b < nb; ++b) w |= (uint32_t)m.h[k + b] << (8u * b);
    return w;
}

// Launch shapes: a wave takes two records (PAIR), or -- batches whose datagrams average ICMP4_LONE_AVG
// bytes or more -- one, member B void: a long answer is one wave's whole latency chain, and twice the
// waves hide it better (measured at two points, 29360 x 9000 and 4096 x 64512 bytes:
// profiles/icmp4/ab_shapes.txt; the threshold itself is not measured).  Results never depend on the shape.
// ICMP4_U 64-unit rows a step (3: two 1480-byte transports).
constexpr uint64_t ICMP4_LONE_AVG = 1024u;

template <uint32_t ICMP4_U, bool PAIR>
__global__ __launch_bounds__(256) void icmp4_answer_kernel(Icmp4Args p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = uni64((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint64_t iA = PAIR ? 2u * w : w, iB = iA + 1u;
    if (iA >= p.n) return;
    const Icmp4Member A = icmp4_member(p, iA, true), B = icmp4_member(p, iB, PAIR && iB < p.n);
    if (!A.on && !B.on) return;

    uint32_t nbA, nbB;
    const uint32_t wA = icmp4_word(A, lane, nbA), wB = icmp4_word(B, lane, nbB);
    // pico_icmp4_checksum: the ICMP header's words and a notice's quote here, an echo's bytes 4 .. T
    // as the mover copies them
    uint32_t accA = lane >= 5u && nbA ? halves(wA) : 0u, accB = lane >= 5u && nbB ? halves(wB) : 0u;
    unit_pair_move<ICMP4_U, false, true>(A.s, B.s, A.echo ? A.d + 24u : 0u, B.echo ? B.d + 24u : 0u, A.e, B.e, A.pl, B.pl,
                                         B.on, lane, accA, accB);
    const uint32_t crcA = finalize(wave_total(accA));
    const uint32_t crcB = finalize(wave_total(accB));

#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const uint32_t nb = b ? nbB : nbA;
        if (nb == 0u) continue;
        uint32_t v = b ? wB : wA;
        if (lane == 5u) v |= bswap16(b ? crcB : crcA) << 16;
        store_word(reinterpret_cast<uint8_t*>(b ? B.d : A.d) + 4u * lane, v, nb);
    }
}

}  // namespace

extern "C" {

int pico_csum_launch_icmp4_reply(const void* base, uint64_t base_len, const void* desc, uint32_t n, const void* req,
                                 void* state, void* out, uint64_t out_len, const void* out_desc, void* o_ans,
                                 uint8_t* verdict, void* stream) {
    if (n == 0) return (int)hipSuccess;
    if (!verdict) return (int)hipErrorInvalidValue;
    Icmp4Args a{static_cast<const uint8_t*>(base), base_len, static_cast<const pico_csum_desc_dev*>(desc), n,
                static_cast<const uint32_t*>(req), static_cast<uint32_t*>(state), static_cast<uint8_t*>(out), out_len,
                static_cast<const pico_csum_desc_dev*>(out_desc), static_cast<pico_csum_desc_dev*>(o_ans), verdict};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((uint64_t)n + 255u) / 256u)), block(256);
    const uint64_t pairs = ((uint64_t)n + 1u) / 2u;
    hipLaunchKernelGGL(icmp4_verdict_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(icmp4_dup_kernel, grid, block, 0, s, a);
    if (base_len >= ICMP4_LONE_AVG * n)
        hipLaunchKernelGGL((icmp4_answer_kernel<3u, false>), dim3((unsigned)(((uint64_t)n + 3u) / 4u)), block, 0, s, a);
    else
        hipLaunchKernelGGL((icmp4_answer_kernel<3u, true>), dim3((unsigned)((pairs + 3u) / 4u)), block, 0, s, a);
    if (state) hipLaunchKernelGGL(icmp4_state_kernel, dim3(1), block, 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"
