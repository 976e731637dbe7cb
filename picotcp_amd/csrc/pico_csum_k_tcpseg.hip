// pico_csum_k_tcpseg.hip -- TCP send segmentation (what a NIC calls TSO): one header template and one
// long payload per connection scattered into segment-sized frames, every frame with its own IPv4
// header checksum and TCP checksum, in one pass that reads each payload byte once -- and its
// launcher.  The TCP sibling of the fragmentation scatter (pico_csum_k_fragtx.hip), whose output
// conventions it keeps.  Helpers, the 16-byte unit mover both go through (unit_pair_move), the header
// word's halves and store (halves, store_word) and the arithmetic contract: pico_csum_dev.h.
//
// Reference: pico_socket_xmit (stack/pico_socket.c:1322-1358) loops pico_socket_xmit_one
// (:1070-1127: a frame per `space` bytes, memcpy of the payload); pico_tcp_push
// (modules/pico_tcp.c:3127-3157: seq = snd_last + 1, snd_last += payload_len); pico_tcp_output
// (:2924-2998) with tcp_add_options_frame (:633-660); tcp_send (:968-985: ports, PSH|ACK, ack, rwnd,
// crc = short_be(pico_tcp_checksum(f))); pico_ipv4_frame_push (modules/pico_ipv4.c:1039-1079: len,
// id = ipv4_progressive_id++, frag = DF, pico_ipv4_checksum).  The reference touches every payload
// byte twice (memcpy, pico_tcp_checksum) and every header twice.
//
// One workgroup per stream; every check is made before the first store (a MALFORMED stream writes
// nothing into its region):
//   1. the template, one lane per 32-bit word of its H = N + thl bytes (H <= 100: 25 lanes): the
//      word sums of the IPv4 header without len / id / frag / crc, of the addresses (the pseudo
//      header's address part) and of the TCP header without seq / crc, once per stream;
//   2. wave w takes the segment pairs w, w + 4, ... (one wave: every pair): segments 2j and
//      2j + 1.  The two payloads move through unit_pair_move, every unit's bytes into its OWN
//      segment's sum (the pairing is relative to the segment's payload start, whatever the parity
//      of k per): two accumulators per lane, two wave reductions (DPP) per pair -- no LDS, no
//      barrier; the readable block ends with the stream;
//   3. behind the reductions the wave writes both headers once, complete: the template's words
//      with len, id + k, DF and pico_ipv4_checksum (IPv4) or the payload length (IPv6), seq +
//      k per, and pico_tcp_checksum = the template's sums + the segment's own len / seq words + its
//      payload sum (store_word).
#include "pico_csum_dev.h"

namespace {

struct TcpSegArgs {
    const uint8_t* base;
    uint64_t base_len;
    const pico_csum_desc_dev* strm;     // per stream: template + payload (off, len), seed = payload bytes a segment
    uint32_t n_stream;
    const uint32_t* grp;                // 2 per stream: first slot, slots reserved
    uint32_t n_seg;
    uint32_t stride;
    uint8_t* out;
    uint64_t out_len;
    const pico_csum_desc_dev* odesc;    // per stream: output region (off, capacity)
    pico_csum_desc_dev* o_seg;
    uint32_t* o_count;
    uint8_t* verdict;
};

// Launch shapes, the fragmentation kernel's two (the thresholds: SHORT_GROUPS_MIN /
// SHORT_SLOTS_AVG, pico_csum_dev.h).  Four waves per stream and three 64-unit rows per step; large
// batches of short streams one wave per stream and TCPSEG_SHORT_U rows per step.  Measured for this
// kernel (profiles/tcpseg/ab_shapes.txt): the two shapes and TCPSEG_SHORT_U = 1 / 2 / 3 at ONE
// point, 29360 streams of 7 segments.
constexpr uint32_t TCPSEG_SHORT_U = 1u;

// TSG_WAVES waves per stream, TSG_U 64-unit rows per step (3: two 1448-byte payloads)
template <uint32_t TSG_WAVES, uint32_t TSG_U>
__global__ __launch_bounds__(64 * TSG_WAVES) void tcp_segment_kernel(TcpSegArgs p) {
    const uint32_t g = blockIdx.x;
    if (g >= p.n_stream) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const pico_csum_desc_dev d = p.strm[g], od = p.odesc[g];
    const uint32_t first = p.grp[2 * g], reserved = p.grp[2 * g + 1];
    const uint32_t per = d.seed;

    // ---- checks (workgroup-uniform, in an order that never reads past d.len): nothing is stored
    // for a stream that fails one
    const bool slots_ok = slots_in(first, reserved, p.n_seg);
    bool bad = span_out(d, p.base_len) || d.len < 1u;
    const uint8_t* h = p.base + d.off;
    uint32_t N = 20u, thl = 20u;
    bool v6 = false;
    if (!bad) {
        const uint32_t b0 = h[0];
        v6 = (b0 >> 4) == 6u;
        N = v6 ? 40u : 20u;
        bad = !(v6 || (b0 >> 4) == 4u) || d.len < N;
        if (!bad) bad = v6 ? (uint32_t)h[6] != 6u : ((b0 & 15u) != 5u || (uint32_t)h[9] != 6u);
        bad = bad || d.len < N + 20u;
        if (!bad) {
            thl = 4u * ((uint32_t)h[N + 12u] >> 4);
            bad = thl < 20u || d.len < N + thl;
        }
    }
    const uint32_t H = N + thl;
    const uint32_t P = bad ? 0u : d.len - H;
    bad = bad || per == 0u;
    const uint32_t seg0 = min(per, P);                              // the longest segment's payload
    bad = bad || (uint64_t)(v6 ? thl : H) + seg0 > 65535u || (uint64_t)H + seg0 > p.stride;
    const SlotPlan sp = bad ? SlotPlan{0u, 0u, 0u} : slot_plan(P, per, p.stride, H, P <= per);
    const uint32_t count = sp.count, last_pl = sp.last_pl;
    bad = bad || reserved < count || !slots_ok || span_out(od, p.out_len) || sp.need > od.len;

    if (p.o_seg && slots_ok)
        write_slots(p.o_seg + first, reserved, bad ? 0u : count, od.off, p.stride, H, per, last_pl, tid, 64u * TSG_WAVES);
    if (tid == 0) {
        if (p.o_count) p.o_count[g] = bad ? 0u : count;
        if (p.verdict) p.verdict[g] = (uint8_t)(bad ? V_MALFORMED : V_ACCEPT);
    }
    if (bad) return;

    // ---- 1. the template: lane l holds its 32-bit word l (little-endian, as it lies in memory)
    const uint32_t nw = H >> 2, tw0 = N >> 2;                       // words; the TCP header's first
    uint32_t tw = 0;
    if (lane < nw) __builtin_memcpy(&tw, h + 4u * lane, 4);
    const uint32_t j = lane - tw0;                                  // the word's place in the TCP header
    // IPv4 header without len (word 0 high), id / frag (word 1), crc (word 2 high)
    const uint32_t n_part = !v6 && lane < 5u ? halves(tw, lane != 1u, lane >= 3u) : 0u;
    const uint32_t a_part = (v6 ? lane >= 2u && lane < 10u : lane >= 3u && lane < 5u) ? halves(tw) : 0u;
    // TCP header without seq (word 1) and crc (word 4 low)
    const uint32_t t_part = lane >= tw0 && lane < nw ? halves(tw, j != 1u && j != 4u, j != 1u) : 0u;
    const uint32_t nsum = wave_total(n_part);
    // the pseudo header's constant part (struct pico_ipv4_pseudo_hdr / pico_ipv6_pseudo_hdr as LE
    // words: the addresses, proto 6) and the TCP header's
    const uint32_t csum = wave_total(a_part + t_part) + (6u << 8);
    const uint32_t id0 = bswap16((uint32_t)__builtin_amdgcn_readlane((int)tw, 1) & 0xFFFFu);
    const uint32_t seq0 = __builtin_bswap32((uint32_t)__builtin_amdgcn_readlane((int)tw, (int)(tw0 + 1u)));

    // ---- 2. scatter + per-segment sums, 3. headers
    const uint64_t S = reinterpret_cast<uint64_t>(h) + H;                            // the payload
    const uint64_t a1 = (reinterpret_cast<uint64_t>(h) + d.len + 15u) & ~(uint64_t)15;   // end of its last 16-byte block
    const uint64_t D = reinterpret_cast<uint64_t>(p.out) + od.off;                   // segment 0's header
    const uint32_t npair = (count + 1u) >> 1;
    for (uint32_t jp = wv; jp < npair; jp += TSG_WAVES) {
        const uint32_t kA = 2u * jp, kB = kA + 1u;
        const bool hasB = kB < count;
        const uint32_t plA = kA + 1u < count ? per : last_pl, plB = hasB ? (kB + 1u < count ? per : last_pl) : 0u;
        const uint64_t dA = D + (uint64_t)kA * p.stride, dB = D + (uint64_t)kB * p.stride;
        const uint64_t sA = S + (uint64_t)kA * per, sB = S + (uint64_t)kB * per;

        uint32_t accA = 0, accB = 0;
        unit_pair_move<TSG_U, false, true>(sA, sB, dA + H, dB + H, a1, a1, plA, plB, hasB, lane, accA, accB);
        const uint32_t payA = wave_total(accA);
        const uint32_t payB = wave_total(accB);

        // the headers: the template's words with the segment's own fields
        if (lane < nw) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if (b == 1 && !hasB) break;
                const uint32_t k = b ? kB : kA, pl = b ? plB : plA;
                const uint32_t seq = seq0 + (uint32_t)((uint64_t)k * per);
                const uint32_t tlen = bswap16(thl + pl);                             // the pseudo header's length word
                const uint32_t tcrc = finalize(csum + tlen + bswap16(seq >> 16) + bswap16(seq & 0xFFFFu) + (b ? payB : payA));
                uint32_t v = tw;
                if (v6) {
                    v = lane == 1u ? (v & 0xFFFF0000u) | tlen : v;                   // payload length
                } else {
                    const uint32_t len = bswap16(H + pl), id = bswap16((id0 + k) & 0xFFFFu);
                    const uint32_t ncrc = finalize(nsum + len + id + 0x0040u);       // frag = 40 00
                    v = lane == 0u ? (v & 0xFFFFu) | (len << 16) : v;
                    v = lane == 1u ? id | (0x0040u << 16) : v;
                    v = lane == 2u ? (v & 0xFFFFu) | (bswap16(ncrc) << 16) : v;
                }
                v = j == 1u ? __builtin_bswap32(seq) : v;
                v = j == 4u ? (v & 0xFFFF0000u) | bswap16(tcrc) : v;
                store_word(reinterpret_cast<uint8_t*>(b ? dB : dA) + 4u * lane, v);
            }
        }
    }
}

}  // namespace

extern "C" {

int pico_csum_launch_tcp_segment(const void* base, uint64_t base_len, const void* strm, uint32_t n_stream,
                                 const uint32_t* groups, uint32_t n_seg, void* out, uint64_t out_len, const void* out_desc,
                                 uint32_t stride, void* o_seg, uint32_t* o_count, uint8_t* verdict, void* stream) {
    if (n_stream == 0) return (int)hipSuccess;
    TcpSegArgs a{static_cast<const uint8_t*>(base), base_len, static_cast<const pico_csum_desc_dev*>(strm), n_stream,
                 groups, n_seg, stride, static_cast<uint8_t*>(out), out_len,
                 static_cast<const pico_csum_desc_dev*>(out_desc), static_cast<pico_csum_desc_dev*>(o_seg), o_count,
                 verdict};
    if (short_groups(n_stream, n_seg))
        hipLaunchKernelGGL((tcp_segment_kernel<1u, TCPSEG_SHORT_U>), dim3(n_stream), dim3(64), 0,
                           static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL((tcp_segment_kernel<4u, 3u>), dim3(n_stream), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // extern "C"
